// Core and extension scans of Panda on bit sets (PyBMF/models/Panda.py:162-334), exact integer work; the fp64 decisions are the
// reference's expressions, products and sums in its order (this file is built with -ffp-contract=off: never an FMA).
//
// rs_t, pd_t: the residual and the cover TRANSPOSED (bit row c = column c of X, ld = m_pad / 32 words); rs, pd: the same row-major
// (bit row r = row r, ldr = n_pad / 32 words); all zero padded.  T: a set of rows (ld words), I: a set of columns (ldr words).
//   couples  score_c = sum of rowcount[r] over the set bits r of rs_t[c], minus |rs_t[c]|                    (panda_couples_kernel)
//   counts   a_i = |T & rs_t[cand[i]]|  (and b_i = |T & pd_t[cand[i]]|) for a block of the list              (panda_count_kernel)
//   core     d_cost(h1) = w_model ((w0 + 1 + h1) - (w0 + h0)) - w_fn ((w0 + 1) h1 - w0 h0):  the FIRST i in list order with
//            d_cost(a_i) <= 0; correlation mode: the pick is the highest a_i, among equals the LAST position, and it wins iff its
//            d_cost <= 0                                                                                      (panda_core_pick_kernel)
//   close    T &= rs_t[winner], |T|                                                                           (panda_close_kernel)
//   ext      cost_new = cost_old + w_model 1 + w_fp (|T| - b_i - a_i) + w_fn (-a_i):  the first i with cost_new <= cost_old
//                                                                                                             (panda_ext_pick_kernel)
//   rows     the winner joins I; for every row r outside T: d_fn = -|rs_r & I|, d_fp = |I| - |pd_r & I| + d_fn,
//            d = w_model 1 + (w_fn d_fn + w_fp d_fp), rows with d <= 0 join T; their number and the sums of d_fn and d_fp
//                                                                                  (panda_item_kernel, panda_rows_kernel, panda_join_kernel)
// Integer adds in a fixed order, no atomics: the same input gives the same output whatever the grid.
#include "bits_common.h"

namespace {

__device__ inline long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the block's sum of v in thread 0 (256 threads; red: 256 int64 of LDS); ends with a barrier
__device__ inline long long block_sum_256(long long v, long long* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    const long long s = red[0];
    __syncthreads();
    return s;
}

// One wave per column, 4 columns per block.  A set bit beyond row m (there is none in a zero padded matrix) is not followed.
__global__ __launch_bounds__(256) void panda_couples_kernel(const uint32_t* __restrict__ rs_t, int n, int ld, const int32_t* __restrict__ rowcount,
                                                            int m, int64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n) return;
    const uint32_t* r = rs_t + (int64_t)c * ld;
    long long s = 0;
    uint32_t cnt = 0;
    for (int w = lane; w < ld; w += 64) {
        uint32_t v = r[w];
        cnt += __popc(v);
        while (v) {
            const int row = w * 32 + __ffs(v) - 1;
            v &= v - 1;
            if (row < m) s += rowcount[row];
        }
    }
    s = wave_sum_i64(s);
    cnt = wave_sum(cnt);
    if (lane == 0) out[c] = (int64_t)s - (int64_t)cnt;
}

// One wave per candidate, 4 per block, 16-byte loads: a[i] = |A[cand[i]] & T|, and b[i] = |B[cand[i]] & T| when B is given.
// A candidate outside [0, n) counts 0 (the host never lists one).
__global__ __launch_bounds__(256) void panda_count_kernel(const uint4* __restrict__ A, const uint4* __restrict__ B, int n, int ld4,
                                                          const uint4* __restrict__ T, const int32_t* __restrict__ cand, int count,
                                                          int32_t* __restrict__ a, int32_t* __restrict__ b) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= count) return;
    const int col = cand[i];
    uint32_t ca = 0, cb = 0;
    if (col >= 0 && col < n) {
        const int64_t base = (int64_t)col * ld4;
#pragma unroll 2
        for (int w = lane; w < ld4; w += 64) {
            const uint4 tv = T[w];
            ca += popc4(and4(A[base + w], tv));
            if (B) cb += popc4(and4(B[base + w], tv));
        }
        ca = wave_sum(ca);
        cb = wave_sum(cb);
    }
    if (lane == 0) {
        a[i] = (int32_t)ca;
        if (B) b[i] = (int32_t)cb;
    }
}

__device__ inline double core_d_cost(double w_model, double w_fn, double w0, double h0, double h1) {
    const double w1 = w0 + 1.0;
    return w_model * ((w1 + h1) - (w0 + h0)) - w_fn * ((w1 * h1) - (w0 * h0));
}

// One block.  rec[0] = the winner's position (-1: none), rec[1] = its column, rec[2] = its h1, rec[3] = the pick's position (mode 0:
// the winner's), rec[4..7] = 0.
__global__ __launch_bounds__(256) void panda_core_pick_kernel(const int32_t* __restrict__ h1, const int32_t* __restrict__ cand, int count, int mode,
                                                              double w_model, double w_fn, double w0, double h0, int64_t* __restrict__ rec) {
    __shared__ long long red[256];
    const int t = threadIdx.x;
    long long key;
    if (mode == 0) {
        key = count;                                      // the smallest qualifying position
        for (int i = t; i < count; i += 256)
            if (core_d_cost(w_model, w_fn, w0, h0, (double)h1[i]) <= 0.0) {
                key = i;
                break;
            }
    } else {
        key = -1;                                         // the largest (h1, position)
        for (int i = t; i < count; i += 256) {
            const long long k = ((long long)h1[i] << 32) | (long long)i;
            key = k > key ? k : key;
        }
    }
    red[t] = key;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] = mode == 0 ? (red[t + o] < red[t] ? red[t + o] : red[t]) : (red[t + o] > red[t] ? red[t + o] : red[t]);
        __syncthreads();
    }
    if (t == 0) {
        int pick = mode == 0 ? (red[0] < count ? (int)red[0] : -1) : (int)(red[0] & 0x7fffffffLL);
        int win = pick;
        if (mode != 0 && !(core_d_cost(w_model, w_fn, w0, h0, (double)h1[pick]) <= 0.0)) win = -1;
        rec[0] = win;
        rec[1] = win >= 0 ? cand[win] : -1;
        rec[2] = win >= 0 ? h1[win] : 0;
        rec[3] = pick;
        rec[4] = rec[5] = rec[6] = rec[7] = 0;
    }
}

// One block.  col = j, or rec[1] when j < 0 (nothing is intersected when that is -1 or outside [0, n)); T &= rs_t[col]; rec[4] = |T|.
__global__ __launch_bounds__(256) void panda_close_kernel(const uint32_t* __restrict__ rs_t, int n, int ld, int j, int64_t* __restrict__ rec,
                                                          uint32_t* __restrict__ T) {
    __shared__ long long red[256];
    const int64_t col = j >= 0 ? j : rec[1];
    const bool take = col >= 0 && col < n;
    long long c = 0;
    for (int w = threadIdx.x; w < ld; w += 256) {
        uint32_t v = T[w];
        if (take) {
            v &= rs_t[col * ld + w];
            T[w] = v;
        }
        c += __popc(v);
    }
    c = block_sum_256(c, red);
    if (threadIdx.x == 0) rec[4] = c;
}

// One block.  rec[0] = the position of the first candidate with cost_new <= cost_old (-1: none), rec[1] = its column, rec[2] = its
// a, rec[3] = its b, rec[4..7] = 0.
__global__ __launch_bounds__(256) void panda_ext_pick_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                             const int32_t* __restrict__ cand, int count, double n_t, double w_model, double w_fp,
                                                             double w_fn, double cost_old, int64_t* __restrict__ rec) {
    __shared__ long long red[256];
    const int t = threadIdx.x;
    long long key = count;
    for (int i = t; i < count; i += 256) {
        const double partial_fn = -(double)a[i];
        const double partial_fp = n_t - (double)b[i] + partial_fn;
        const double cost_new = cost_old + w_model * 1.0 + w_fp * partial_fp + w_fn * partial_fn;
        if (cost_new <= cost_old) {
            key = i;
            break;
        }
    }
    red[t] = key;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] = red[t + o] < red[t] ? red[t + o] : red[t];
        __syncthreads();
    }
    if (t == 0) {
        const int win = red[0] < count ? (int)red[0] : -1;
        rec[0] = win;
        rec[1] = win >= 0 ? cand[win] : -1;
        rec[2] = win >= 0 ? a[win] : 0;
        rec[3] = win >= 0 ? b[win] : 0;
        rec[4] = rec[5] = rec[6] = rec[7] = 0;
    }
}

// the column that joins I: j, or rec[1] when j < 0; -1 when there is none
__device__ inline int64_t joining_column(int j, const int64_t* rec, int n) {
    const int64_t col = j >= 0 ? j : rec[1];
    return col >= 0 && col < n ? col : -1;
}

__global__ void panda_item_kernel(int j, const int64_t* __restrict__ rec, int n, uint32_t* __restrict__ I) {
    const int64_t col = joining_column(j, rec, n);
    if (col >= 0) I[col >> 5] |= 1u << (col & 31);
}

// One wave per row, 4 rows per block, 16-byte loads.  p[r] = |rs_r & I|, q[r] = |pd_r & I|, join[r] = (r outside T and d <= 0).
// Nothing is written when no column joins I.
__global__ __launch_bounds__(256) void panda_rows_kernel(const uint4* __restrict__ rs, const uint4* __restrict__ pd, int m, int ldr4, int n, int j,
                                                         const int64_t* __restrict__ rec, const uint4* __restrict__ I, double n_i,
                                                         const uint32_t* __restrict__ T, double w_model, double w_fp, double w_fn,
                                                         int32_t* __restrict__ join, int32_t* __restrict__ p, int32_t* __restrict__ q) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= m || joining_column(j, rec, n) < 0) return;
    const int64_t base = (int64_t)r * ldr4;
    uint32_t cp = 0, cq = 0;
#pragma unroll 2
    for (int w = lane; w < ldr4; w += 64) {
        const uint4 iv = I[w];
        cp += popc4(and4(rs[base + w], iv));
        cq += popc4(and4(pd[base + w], iv));
    }
    cp = wave_sum(cp);
    cq = wave_sum(cq);
    if (lane == 0) {
        const double d_fn = -(double)cp;
        const double d_fp = n_i - (double)cq + d_fn;
        const double d = w_model * 1.0 + (w_fn * d_fn + w_fp * d_fp);
        const bool in_t = (T[r >> 5] >> (r & 31)) & 1u;
        join[r] = (!in_t && d <= 0.0) ? 1 : 0;
        p[r] = (int32_t)cp;
        q[r] = (int32_t)cq;
    }
}

// One block.  The rows that join are set in T; out[0] = their number, out[1] = sum of d_fn = -p, out[2] = sum of d_fp = n_i - q - p
// over them, out[3] = 0.  All zero, T untouched, when no column joined I.
__global__ __launch_bounds__(256) void panda_join_kernel(int m, int ldt, int n, int j, const int64_t* __restrict__ rec, long long n_i,
                                                         const int32_t* __restrict__ join, const int32_t* __restrict__ p,
                                                         const int32_t* __restrict__ q, uint32_t* __restrict__ T, int64_t* __restrict__ out) {
    __shared__ long long red[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool active = joining_column(j, rec, n) >= 0;        // (block-uniform)
    long long added = 0, s_fn = 0, s_fp = 0;
    if (active) {
        for (int r0 = 0; r0 < m; r0 += 256) {
            const int r = r0 + tid;
            const bool in = r < m && join[r] != 0;
            if (in) {
                added += 1;
                s_fn -= p[r];
                s_fp += n_i - q[r] - p[r];
            }
            const unsigned long long bits = __ballot(in);
            const int word = (r0 >> 5) + wave * 2;
            if (lane == 0 && word < ldt && (uint32_t)bits) T[word] |= (uint32_t)bits;
            if (lane == 32 && word + 1 < ldt && (uint32_t)(bits >> 32)) T[word + 1] |= (uint32_t)(bits >> 32);
        }
    }
    added = block_sum_256(added, red);
    s_fn = block_sum_256(s_fn, red);
    s_fp = block_sum_256(s_fp, red);
    if (tid == 0) {
        out[0] = added;
        out[1] = s_fn;
        out[2] = s_fp;
        out[3] = 0;
    }
}

}  // namespace

extern "C" int bmf_panda_couples(const uint32_t* rs_t, int32_t n, int64_t ld, const int32_t* rowcount, int32_t m, int64_t* out, void* stream) {
    BMF_REQUIRE(rs_t && rowcount && out, "bmf_panda_couples: null pointer");
    BMF_REQUIRE(n >= 1 && m >= 1 && ld >= 1 && ld <= (1 << 26), "bmf_panda_couples: need n >= 1, m >= 1 and 1 <= ld <= 2^26");
    BMF_REQUIRE((int64_t)m <= 32 * ld, "bmf_panda_couples: m rows need m <= 32 * ld");
    BMF_LAUNCH(panda_couples_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rs_t, n, (int)ld, rowcount, m, out);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_panda_core_scan(const uint32_t* rs_t, int32_t n, int64_t ld, const uint32_t* T, const int32_t* cand, int32_t count,
                                   int32_t mode, double w_model, double w_fn, int64_t w0, int64_t h0, int32_t* h1, int64_t* rec,
                                   void* stream) {
    BMF_REQUIRE(rs_t && T && cand && h1 && rec, "bmf_panda_core_scan: null pointer");
    BMF_REQUIRE(n >= 1 && count >= 1, "bmf_panda_core_scan: need n >= 1 and count >= 1");
    BMF_REQUIRE(ld_ok(ld), "bmf_panda_core_scan: ld must be a multiple of 4 words, at most 2^26");
    BMF_REQUIRE(mode == 0 || mode == 1, "bmf_panda_core_scan: mode is 0 (first in list order) or 1 (correlation pick)");
    BMF_REQUIRE(w0 >= 1 && h0 >= 0, "bmf_panda_core_scan: need w0 >= 1 items and h0 >= 0 transactions");
    BMF_REQUIRE(bmf_aligned16(rs_t) && bmf_aligned16(T), "bmf_panda_core_scan: rs_t and T must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(panda_count_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const uint4*>(rs_t),
               static_cast<const uint4*>(nullptr), n, (int)(ld / 4), reinterpret_cast<const uint4*>(T), cand, count, h1, static_cast<int32_t*>(nullptr));
    BMF_LAUNCH(panda_core_pick_kernel, dim3(1), dim3(256), 0, s, h1, cand, count, mode, w_model, w_fn, (double)w0, (double)h0, rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_panda_close(const uint32_t* rs_t, int32_t n, int64_t ld, int32_t j, int64_t* rec, uint32_t* T, void* stream) {
    BMF_REQUIRE(rs_t && rec && T, "bmf_panda_close: null pointer");
    BMF_REQUIRE(n >= 1 && ld >= 1 && ld <= (1 << 26), "bmf_panda_close: need n >= 1 and 1 <= ld <= 2^26");
    BMF_REQUIRE(j < n, "bmf_panda_close: column j must be below n (negative: the column of rec)");
    BMF_LAUNCH(panda_close_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, rs_t, n, (int)ld, j, rec, T);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_panda_ext_scan(const uint32_t* rs_t, const uint32_t* pd_t, int32_t n, int64_t ld, const uint32_t* T, const int32_t* cand,
                                  int32_t count, int64_t n_t, double w_model, double w_fp, double w_fn, double cost_old, int32_t* a,
                                  int32_t* b, int64_t* rec, void* stream) {
    BMF_REQUIRE(rs_t && pd_t && T && cand && a && b && rec, "bmf_panda_ext_scan: null pointer");
    BMF_REQUIRE(n >= 1 && count >= 1 && n_t >= 0, "bmf_panda_ext_scan: need n >= 1, count >= 1 and n_t >= 0");
    BMF_REQUIRE(ld_ok(ld), "bmf_panda_ext_scan: ld must be a multiple of 4 words, at most 2^26");
    BMF_REQUIRE(bmf_aligned16(rs_t) && bmf_aligned16(pd_t) && bmf_aligned16(T), "bmf_panda_ext_scan: rs_t, pd_t and T must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(panda_count_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const uint4*>(rs_t),
               reinterpret_cast<const uint4*>(pd_t), n, (int)(ld / 4), reinterpret_cast<const uint4*>(T), cand, count, a, b);
    BMF_LAUNCH(panda_ext_pick_kernel, dim3(1), dim3(256), 0, s, a, b, cand, count, (double)n_t, w_model, w_fp, w_fn, cost_old, rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int64_t bmf_panda_rows_work(int32_t m) {
    if (m < 1) return BMF_ERR_BAD_ARG;
    return (int64_t)m * 12;   // bytes: int32 join, p, q per row
}

extern "C" int bmf_panda_rows(const uint32_t* rs, const uint32_t* pd, int32_t m, int64_t ldr, int32_t n, int32_t j, const int64_t* rec,
                              uint32_t* I, int64_t n_i, uint32_t* T, int64_t ldt, double w_model, double w_fp, double w_fn, void* work,
                              int64_t* out, void* stream) {
    BMF_REQUIRE(rs && pd && rec && I && T && work && out, "bmf_panda_rows: null pointer");
    BMF_REQUIRE(m >= 1 && n >= 1 && n_i >= 1, "bmf_panda_rows: need m >= 1, n >= 1 and n_i >= 1");
    BMF_REQUIRE(ld_ok(ldr), "bmf_panda_rows: ldr must be a multiple of 4 words, at most 2^26");
    BMF_REQUIRE(ldt >= 1 && ldt <= (1 << 26) && (int64_t)m <= 32 * ldt, "bmf_panda_rows: T needs 1 <= ldt <= 2^26 and m <= 32 * ldt");
    BMF_REQUIRE((int64_t)n <= 32 * ldr, "bmf_panda_rows: n columns need n <= 32 * ldr");
    BMF_REQUIRE(j < n, "bmf_panda_rows: column j must be below n (negative: the column of rec)");
    BMF_REQUIRE(bmf_aligned16(rs) && bmf_aligned16(pd) && bmf_aligned16(I), "bmf_panda_rows: rs, pd and I must be 16-byte aligned");
    BMF_REQUIRE((reinterpret_cast<uintptr_t>(work) & 3u) == 0, "bmf_panda_rows: work must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    int32_t* join = static_cast<int32_t*>(work);
    int32_t *p = join + m, *q = join + 2 * (int64_t)m;
    BMF_LAUNCH(panda_item_kernel, dim3(1), dim3(1), 0, s, j, rec, n, I);
    BMF_LAUNCH(panda_rows_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const uint4*>(rs), reinterpret_cast<const uint4*>(pd), m,
               (int)(ldr / 4), n, j, rec, reinterpret_cast<const uint4*>(I), (double)n_i, T, w_model, w_fp, w_fn, join, p, q);
    BMF_LAUNCH(panda_join_kernel, dim3(1), dim3(256), 0, s, m, (int)ldt, n, j, rec, (long long)n_i, join, p, q, T, out);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
