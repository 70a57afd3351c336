// The two refiners of an Asso model (PyBMF/models/AssoIter.py, AssoOpt.py): U is re-decided against fixed V, one column at a time
// (AssoIter) or one row at a time over all 2^k subsets of the factors (AssoOpt).  Same kind of work as asso.hip: AND / OR-popcount over
// bit rows, exact integer counts, the reference's fp64 expression (-w_fp) FP + w_fn TP on them (two products, one sum, no FMA), partial
// sums added in a fixed order, no atomics: the same input gives the same bytes.
//
// X: row-major bits, ldx = n_pad / 32 words per row (a multiple of 16).  V: one bit row of ldx words per FACTOR (k rows).  U: one mask
// of kw = ceil(k / 32) words per row of X, bit l of the mask = U[r][l]; bits >= k are ignored.
//
// The bit rows of V sit in LDS `chunk` words at a time (row stride chunk + 4 words: rows of different factors read by the lanes of one
// wave fall into different 16-byte slots).  A workgroup's LDS is kept within 64 KiB by choice (two workgroups and more per CU of the
// 160 KiB): chunk = ldx when k n_pad bits fit, else the kernels walk over n chunk by chunk and keep their per-row counts in registers.
//
// refine_column_kernel  32 rows per workgroup = one word of the new column, 8 lanes per row, each on every 8th group of 4 words.  Per
//                       row: X_old = OR of the V rows its mask selects, factor kc left out; X_new = X_old | V[kc];  TP / FP of both
//                       against x_r by popcount; the row takes V[kc] iff score(new) > score(old), strict.  Bit kc of the row's mask
//                       and the packed column are written; per workgroup the sums of the chosen TP, FP and the taken rows.
// refine_rows_kernel    one workgroup per row.  Subset j of the factors, factor 0 the most significant bit of j (k bits), is split
//                       as j = [outer bits | thread bits (up to 8) | leaf bits (up to 4)]: a thread ORs the V words of its own bits
//                       once per word (every lane reads the same LDS address: a broadcast) and walks its 16 leaves over them in
//                       registers -- a depth-first walk of the subsets whose stack of partial ORs is the registers of the thread.
//                       The thread keeps its first maximal j (ascending j, strict >), the workgroup the largest score with the
//                       smallest j of equals: NumPy's argmax over scores[0 .. 2^k).
// refine_reduce_kernel  adds the (T, F, count) triples in a fixed order into one record { bits of w_fn T - w_fp F, T, F, count }.
// refine_product_kernel PD_r = OR of the V rows that the mask of row r selects.
#include "common.h"

namespace {

constexpr int LDS_BYTES = 60 << 10;   // of staged bit rows per workgroup: with the reduction arrays within 64 KiB, by choice (the CU has 160)
constexpr int PAD = 4;                // words between LDS rows
constexpr int K_MAX_COLUMN = 1024;    // 1024 LDS rows of 8 + 4 words are 48 KiB: a chunk is never shorter than 8 words
constexpr int K_MAX_ROWS = 16;
constexpr int LEAF_BITS = 4, THREAD_BITS = 8;
constexpr int NO_J = 0x7fffffff;

// the reference's row score, exactly as it is written there: (-w_fp) * FP + w_fn * TP
__device__ __forceinline__ double row_score(double w_fp, double w_fn, double tp, double fp) {
    return __dadd_rn(__dmul_rn(-w_fp, fp), __dmul_rn(w_fn, tp));
}

__device__ __forceinline__ uint32_t popc4(u32x4 a) { return __popc(a[0]) + __popc(a[1]) + __popc(a[2]) + __popc(a[3]); }

// rows [0, rows) of V, words [c0, c0 + cw), into LDS rows of `ld` words; cw is a multiple of 4
__device__ __forceinline__ void stage_rows(uint32_t* sv, int ld, const uint32_t* __restrict__ V, int ldx, int rows, int c0, int cw) {
    const int groups = cw >> 2;
    for (int i = threadIdx.x; i < rows * groups; i += 256) {
        const int l = i / groups, g = i - l * groups;
        *reinterpret_cast<u32x4*>(&sv[l * ld + 4 * g]) = *reinterpret_cast<const u32x4*>(&V[(int64_t)l * ldx + c0 + 4 * g]);
    }
}

// grid ceil(m / 32), block 256, dynamic LDS k * (chunk + PAD) words
__global__ __launch_bounds__(256) void refine_column_kernel(const uint32_t* __restrict__ X, int ldx, int m, const uint32_t* __restrict__ V,
                                                            int k, uint32_t* __restrict__ U, int kw, int kc, int chunk, double w_fp,
                                                            double w_fn, uint32_t* __restrict__ u_out, int64_t* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sv[];
    __shared__ uint32_t flag[32], row_t[32], row_f[32];
    const int t = threadIdx.x, lr = t >> 3, sub = t & 7;
    const int r = blockIdx.x * 32 + lr;
    const bool row_in = r < m;
    const int ld = chunk + PAD;
    const uint32_t* mask = U + (int64_t)(row_in ? r : 0) * kw;
    const uint32_t last = (k & 31) ? (1u << (k & 31)) - 1u : 0xffffffffu;   // the mask bits of the last word that are factors
    uint32_t tp_old = 0, n_old = 0, tp_new = 0, n_new = 0;
    for (int c0 = 0; c0 < ldx; c0 += chunk) {
        const int cw = min(chunk, ldx - c0);
        __syncthreads();                                   // the previous chunk has been read
        stage_rows(sv, ld, V, ldx, k, c0, cw);
        __syncthreads();
        if (row_in)
            for (int g = sub; g < (cw >> 2); g += 8) {
                u32x4 old = {0, 0, 0, 0};
                for (int w = 0; w < kw; ++w) {
                    uint32_t bits = mask[w];
                    if (w == kw - 1) bits &= last;
                    if (w == (kc >> 5)) bits &= ~(1u << (kc & 31));
                    while (bits) {
                        const int l = 32 * w + __ffs(bits) - 1;
                        bits &= bits - 1;
                        old |= *reinterpret_cast<const u32x4*>(&sv[l * ld + 4 * g]);
                    }
                }
                const u32x4 x = *reinterpret_cast<const u32x4*>(&X[(int64_t)r * ldx + c0 + 4 * g]);
                const u32x4 neu = old | *reinterpret_cast<const u32x4*>(&sv[kc * ld + 4 * g]);
                tp_old += popc4(x & old);
                n_old += popc4(old);
                tp_new += popc4(x & neu);
                n_new += popc4(neu);
            }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        tp_old += __shfl_xor(tp_old, o);
        n_old += __shfl_xor(n_old, o);
        tp_new += __shfl_xor(tp_new, o);
        n_new += __shfl_xor(n_new, o);
    }
    if (sub == 0) {
        bool take = false;
        uint32_t ct = 0, cf = 0;
        if (row_in) {
            const uint32_t fp_old = n_old - tp_old, fp_new = n_new - tp_new;
            take = row_score(w_fp, w_fn, (double)tp_new, (double)fp_new) > row_score(w_fp, w_fn, (double)tp_old, (double)fp_old);
            ct = take ? tp_new : tp_old;
            cf = take ? fp_new : fp_old;
            // every read of this row's mask was made by this wave, before the shuffles above
            uint32_t* word = U + (int64_t)r * kw + (kc >> 5);
            *word = take ? (*word | (1u << (kc & 31))) : (*word & ~(1u << (kc & 31)));
        }
        flag[lr] = take ? 1u : 0u;
        row_t[lr] = ct;
        row_f[lr] = cf;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t word = 0;
        int64_t T = 0, F = 0;
#pragma unroll
        for (int q = 0; q < 32; ++q) {
            word |= flag[q] << q;
            T += row_t[q];
            F += row_f[q];
        }
        u_out[blockIdx.x] = word;
        part[3 * (int64_t)blockIdx.x] = T;
        part[3 * (int64_t)blockIdx.x + 1] = F;
        part[3 * (int64_t)blockIdx.x + 2] = __popc(word);
    }
}

// grid m, block 256, dynamic LDS (k + 1) * (chunk + PAD) words: the V rows and, as row k, the row of X
__global__ __launch_bounds__(256) void refine_rows_kernel(const uint32_t* __restrict__ X, int ldx, int m, const uint32_t* __restrict__ V,
                                                          int k, int chunk, double w_fp, double w_fn, int32_t* __restrict__ j_out,
                                                          uint32_t* __restrict__ U, int64_t* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sv[];
    __shared__ double top_s[256];
    __shared__ int top_j[256];
    const int t = threadIdx.x, r = blockIdx.x;
    const int ld = chunk + PAD;
    const int lb = min(LEAF_BITS, k), hb = min(THREAD_BITS, k - lb), ob = k - lb - hb;
    const bool active = t < (1 << hb);
    // factor of leaf bit b: k - 1 - b;  of thread bit b: k - 1 - lb - b;  of outer bit b: k - 1 - lb - hb - b
    const uint32_t* sx = sv + k * ld;
    double best_s = 0.0;
    int best_j = NO_J;
    uint32_t best_tp = 0, best_fp = 0;
    for (int o = 0; o < (1 << ob); ++o) {
        uint32_t tp[16] = {}, np[16] = {};
        for (int c0 = 0; c0 < ldx; c0 += chunk) {
            const int cw = min(chunk, ldx - c0);
            if (o == 0 || chunk < ldx) {                   // one chunk: it stays in LDS for every o
                __syncthreads();
                stage_rows(sv, ld, V, ldx, k, c0, cw);
                stage_rows(sv + k * ld, ld, X + (int64_t)r * ldx, ldx, 1, c0, cw);
                __syncthreads();
            }
            if (active)
                for (int w = 0; w < cw; ++w) {
                    const uint32_t x = sx[w];
                    uint32_t base = 0;
                    for (int b = 0; b < ob; ++b)
                        if ((o >> b) & 1) base |= sv[(k - 1 - lb - hb - b) * ld + w];
                    for (int b = 0; b < hb; ++b) {
                        const uint32_t v = sv[(k - 1 - lb - b) * ld + w];
                        base |= ((t >> b) & 1) ? v : 0u;
                    }
                    uint32_t lw[LEAF_BITS];
#pragma unroll
                    for (int b = 0; b < LEAF_BITS; ++b) lw[b] = b < lb ? sv[(k - 1 - b) * ld + w] : 0u;
                    uint32_t acc[16];
                    acc[0] = base;
#pragma unroll
                    for (int q = 1; q < 16; ++q) {         // leaf q = leaf q without its top bit, OR that bit's factor
                        const int top = 31 - __builtin_clz(q);
                        acc[q] = acc[q & ~(1 << top)] | lw[top];
                    }
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        tp[q] += __popc(x & acc[q]);
                        np[q] += __popc(acc[q]);
                    }
                }
        }
        if (active) {
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (q < (1 << lb)) {                       // ascending j: an equal later score does not replace
                    const uint32_t fp = np[q] - tp[q];
                    const double s = row_score(w_fp, w_fn, (double)tp[q], (double)fp);
                    if (best_j == NO_J || s > best_s) {
                        best_s = s;
                        best_j = (o << (hb + lb)) | (t << lb) | q;
                        best_tp = tp[q];
                        best_fp = fp;
                    }
                }
        }
    }
    top_s[t] = best_s;
    top_j[t] = best_j;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            const double s2 = top_s[t + o];
            const int j2 = top_j[t + o];
            if (j2 != NO_J && (top_j[t] == NO_J || s2 > top_s[t] || (s2 == top_s[t] && j2 < top_j[t]))) {
                top_s[t] = s2;
                top_j[t] = j2;
            }
        }
        __syncthreads();
    }
    if (active && best_j == top_j[0]) {                    // (every j belongs to one thread)
        j_out[r] = best_j;
        U[r] = __brev((uint32_t)best_j) >> (32 - k);       // bit l of the mask = bit k - 1 - l of j
        part[3 * (int64_t)r] = best_tp;
        part[3 * (int64_t)r + 1] = best_fp;
        part[3 * (int64_t)r + 2] = __popc((uint32_t)best_j);
    }
}

// One block: rec = { the bits of w_fn T - w_fp F, T, F, count }, the triples added in a fixed order.
__global__ __launch_bounds__(256) void refine_reduce_kernel(const int64_t* __restrict__ part, int count, double w_fp, double w_fn,
                                                            int64_t* __restrict__ rec) {
    __shared__ int64_t red[3][256];
    const int t = threadIdx.x;
    int64_t s0 = 0, s1 = 0, s2 = 0;
    for (int i = t; i < count; i += 256) {
        s0 += part[3 * (int64_t)i];
        s1 += part[3 * (int64_t)i + 1];
        s2 += part[3 * (int64_t)i + 2];
    }
    red[0][t] = s0;
    red[1][t] = s1;
    red[2][t] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            red[0][t] += red[0][t + o];
            red[1][t] += red[1][t + o];
            red[2][t] += red[2][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        rec[0] = __double_as_longlong(__dsub_rn(__dmul_rn(w_fn, (double)red[0][0]), __dmul_rn(w_fp, (double)red[1][0])));
        rec[1] = red[0][0];
        rec[2] = red[1][0];
        rec[3] = red[2][0];
    }
}

// one wave per row, 4 rows per block
__global__ __launch_bounds__(256) void refine_product_kernel(const uint32_t* __restrict__ U, int kw, const uint32_t* __restrict__ V, int k,
                                                             int ldx, int m, uint32_t* __restrict__ PD) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= m) return;
    const uint32_t last = (k & 31) ? (1u << (k & 31)) - 1u : 0xffffffffu;
    for (int w0 = lane; w0 < ldx; w0 += 64) {
        uint32_t acc = 0;
        for (int w = 0; w < kw; ++w) {
            uint32_t bits = U[(int64_t)r * kw + w];
            if (w == kw - 1) bits &= last;
            while (bits) {
                const int l = 32 * w + __ffs(bits) - 1;
                bits &= bits - 1;
                acc |= V[(int64_t)l * ldx + w0];
            }
        }
        PD[(int64_t)r * ldx + w0] = acc;
    }
}

// words of a bit row per LDS chunk for `rows` LDS rows: all ldx if they fit, else the largest multiple of 4 that does
int chunk_for(int rows, int64_t ldx) {
    const int64_t fit = (LDS_BYTES / 4 / rows - PAD) / 4 * 4;
    return (int)(fit < ldx ? fit : ldx);
}

}  // namespace

extern "C" int bmf_asso_refine_chunk(int32_t k, int64_t ldx, int32_t rows_kernel) {
    const int k_max = rows_kernel ? K_MAX_ROWS : K_MAX_COLUMN;
    if (k < 1 || k > k_max || ldx < 16 || ldx % 16 != 0 || ldx * 32 >= ((int64_t)1 << 31)) return BMF_ERR_BAD_ARG;
    return chunk_for(k + (rows_kernel ? 1 : 0), ldx);
}

extern "C" int bmf_asso_refine_column(const uint32_t* X, int64_t ldx, int32_t m, const uint32_t* V, int32_t k, uint32_t* U, int32_t kw,
                                      int32_t kc, int32_t chunk, double w_fp, double w_fn, uint32_t* u, int64_t* part, int64_t* rec,
                                      void* stream) {
    BMF_REQUIRE(X && V && U && u && part && rec, "bmf_asso_refine_column: null pointer");
    BMF_REQUIRE(m >= 1 && ldx >= 16 && ldx % 16 == 0, "bmf_asso_refine_column: need m >= 1 and ldx a positive multiple of 16");
    BMF_REQUIRE(ldx * 32 < ((int64_t)1 << 31), "bmf_asso_refine_column: too many columns for 32-bit counts");
    BMF_REQUIRE(k >= 1 && k <= K_MAX_COLUMN, "bmf_asso_refine_column: k must be in [1, %d] (8 words of every factor's bit row must fit the %d KiB of LDS a workgroup stages them in)",
                K_MAX_COLUMN, LDS_BYTES >> 10);
    BMF_REQUIRE(kw == (k + 31) / 32 && kc >= 0 && kc < k, "bmf_asso_refine_column: need kw == ceil(k / 32) and 0 <= kc < k");
    BMF_REQUIRE(w_fp == w_fp && w_fn == w_fn, "bmf_asso_refine_column: a weight is not a number");
    BMF_REQUIRE(bmf_aligned16(X) && bmf_aligned16(V), "bmf_asso_refine_column: X and V must be 16-byte aligned");
    const int fit = chunk_for(k, ldx);
    if (chunk == 0) chunk = fit;
    BMF_REQUIRE(chunk >= 4 && chunk % 4 == 0 && chunk <= fit, "bmf_asso_refine_column: chunk must be a multiple of 4 in [4, %d]", fit);
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (m + 31) / 32;
    BMF_LAUNCH(refine_column_kernel, dim3((unsigned)blocks), dim3(256), (size_t)k * (chunk + PAD) * 4, s, X, (int)ldx, m, V, k, U, kw, kc, chunk,
               w_fp, w_fn, u, part);
    BMF_LAUNCH(refine_reduce_kernel, dim3(1), dim3(256), 0, s, part, blocks, w_fp, w_fn, rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_asso_refine_rows(const uint32_t* X, int64_t ldx, int32_t m, const uint32_t* V, int32_t k, int32_t chunk, double w_fp,
                                    double w_fn, int32_t* j, uint32_t* U, int64_t* part, int64_t* rec, void* stream) {
    BMF_REQUIRE(X && V && j && U && part && rec, "bmf_asso_refine_rows: null pointer");
    BMF_REQUIRE(m >= 1 && ldx >= 16 && ldx % 16 == 0, "bmf_asso_refine_rows: need m >= 1 and ldx a positive multiple of 16");
    BMF_REQUIRE(ldx * 32 < ((int64_t)1 << 31), "bmf_asso_refine_rows: too many columns for 32-bit counts");
    BMF_REQUIRE(k >= 1 && k <= K_MAX_ROWS, "bmf_asso_refine_rows: k must be in [1, %d] (2^k subsets per row)", K_MAX_ROWS);
    BMF_REQUIRE(w_fp == w_fp && w_fn == w_fn, "bmf_asso_refine_rows: a weight is not a number");
    BMF_REQUIRE(bmf_aligned16(X) && bmf_aligned16(V), "bmf_asso_refine_rows: X and V must be 16-byte aligned");
    const int fit = chunk_for(k + 1, ldx);
    if (chunk == 0) chunk = fit;
    BMF_REQUIRE(chunk >= 4 && chunk % 4 == 0 && chunk <= fit, "bmf_asso_refine_rows: chunk must be a multiple of 4 in [4, %d]", fit);
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(refine_rows_kernel, dim3((unsigned)m), dim3(256), (size_t)(k + 1) * (chunk + PAD) * 4, s, X, (int)ldx, m, V, k, chunk, w_fp, w_fn,
               j, U, part);
    BMF_LAUNCH(refine_reduce_kernel, dim3(1), dim3(256), 0, s, part, m, w_fp, w_fn, rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_asso_refine_product(const uint32_t* U, int32_t kw, const uint32_t* V, int32_t k, int64_t ldx, int32_t m, uint32_t* PD,
                                       void* stream) {
    BMF_REQUIRE(U && V && PD, "bmf_asso_refine_product: null pointer");
    BMF_REQUIRE(m >= 1 && ldx >= 1 && k >= 1 && kw == (k + 31) / 32, "bmf_asso_refine_product: need m, ldx, k >= 1 and kw == ceil(k / 32)");
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(refine_product_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, U, kw, V, k, (int)ldx, m, PD);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
