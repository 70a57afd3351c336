// Itemset mining and hyperrectangle records of Hyper on bit sets (PyBMF/models/Hyper.py:44-82, 147-186), exact integer work; every
// fp64 decision (the support test, the cost (|T| + |I|) / s and its comparisons) is host arithmetic on the integers written here.
//
// Everything is a bit row over the m rows of X: ld = m_pad / 32 words, zero padded, the layout of the TRANSPOSED matrices (x_t, rs_t:
// bit row j = column j of X, of the residual).  A candidate is an itemset I with its tidset tid = AND of x_t[j] over j in I.
//   level   tid_out[c] = tid_prev[parent_c] & x_t[j_c],  count[c] = |tid_out[c]|      one level of the vertical miner  (hyper_level_kernel)
//   eval    T = tid & OR_{j in I} rs_t[j],  nT = |T|,  s = sum_{j in I} |tid & rs_t[j]|   find_hyper on the residual   (hyper_eval_kernel)
//           (the rows that hold all of I in X and still have a residual one on I; s is what the reference sums over X_rs[T, I])
//   copy    dst[dst_id[i]] = src[src_id[i]]: the commit of scratch T rows, and the compaction of a mined level  (hyper_copy_kernel)
// One wave per candidate, 4 per block, 16-byte loads (a lane takes every 64th uint4 of a row: 1 KiB per wave and load), a wave-level
// sum.  A padding bit is zero in every written row because it is zero in x_t.  No atomics: the same input gives the same output.
#include "bits_common.h"

namespace {

__device__ inline uint4 or4(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }

// pair[2 c] = the parent's slot in tid_prev (< n_prev), pair[2 c + 1] = the column (< n); a pair outside gives an empty row.
__global__ __launch_bounds__(256) void hyper_level_kernel(const uint4* __restrict__ tid_prev, int n_prev, const uint4* __restrict__ x_t, int n,
                                                          int ld4, const int32_t* __restrict__ pair, int count, uint4* __restrict__ tid_out,
                                                          int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= count) return;
    const int p = pair[2 * c], j = pair[2 * c + 1];
    const bool ok = p >= 0 && p < n_prev && j >= 0 && j < n;          // (wave-uniform)
    const int64_t pb = (int64_t)(ok ? p : 0) * ld4, xb = (int64_t)(ok ? j : 0) * ld4, ob = (int64_t)c * ld4;
    uint32_t k = 0;
#pragma unroll 2
    for (int w = lane; w < ld4; w += 64) {
        const uint4 v = ok ? and4(tid_prev[pb + w], x_t[xb + w]) : make_uint4(0u, 0u, 0u, 0u);
        tid_out[ob + w] = v;
        k += popc4(v);
    }
    k = wave_sum(k);
    if (lane == 0) cnt[c] = (int32_t)k;
}

// ids[i] < n_cand names the candidate; items[id * maxlen ..]: its columns, padded with -1.  Writes T_out[id] and rec[2 id] = nT,
// rec[2 id + 1] = s.  An id outside [0, n_cand) writes nothing; a column outside [0, n) counts as an empty one.
__global__ __launch_bounds__(256) void hyper_eval_kernel(const uint4* __restrict__ tid, const uint4* __restrict__ rs_t, int n, int ld4,
                                                         const int32_t* __restrict__ items, int maxlen, const int32_t* __restrict__ ids,
                                                         int count, int n_cand, uint4* __restrict__ T_out, int32_t* __restrict__ rec) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= count) return;
    const int id = ids[i];
    if (id < 0 || id >= n_cand) return;                               // (wave-uniform)
    const int32_t* it = items + (int64_t)id * maxlen;
    const int64_t base = (int64_t)id * ld4;
    uint32_t nT = 0, s = 0;
    for (int w = lane; w < ld4; w += 64) {
        const uint4 t = tid[base + w];
        uint4 any = make_uint4(0u, 0u, 0u, 0u);
        for (int q = 0; q < maxlen; ++q) {
            const int j = it[q];
            if (j < 0) break;
            if (j >= n) continue;
            const uint4 r = rs_t[(int64_t)j * ld4 + w];
            any = or4(any, r);
            s += popc4(and4(t, r));
        }
        const uint4 T = and4(t, any);
        T_out[base + w] = T;
        nT += popc4(T);
    }
    nT = wave_sum(nT);
    s = wave_sum(s);
    if (lane == 0) {
        rec[2 * (int64_t)id] = (int32_t)nT;
        rec[2 * (int64_t)id + 1] = (int32_t)s;
    }
}

// dst[dst_id[i]] = src[src_id[i]] for i < count; a pair with either id outside its array is skipped.
__global__ __launch_bounds__(256) void hyper_copy_kernel(const uint4* __restrict__ src, int n_src, const int32_t* __restrict__ src_id,
                                                         uint4* __restrict__ dst, int n_dst, const int32_t* __restrict__ dst_id, int ld4,
                                                         int count) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= count) return;
    const int a = src_id[i], b = dst_id[i];
    if (a < 0 || a >= n_src || b < 0 || b >= n_dst) return;           // (wave-uniform)
    const int64_t sb = (int64_t)a * ld4, db = (int64_t)b * ld4;
#pragma unroll 2
    for (int w = lane; w < ld4; w += 64) dst[db + w] = src[sb + w];
}

inline bool count_ok(int32_t count) { return count >= 1 && count <= (1 << 30); }

}  // namespace

extern "C" int bmf_hyper_level(const uint32_t* tid_prev, int32_t n_prev, const uint32_t* x_t, int32_t n, int64_t ld, const int32_t* pair,
                               int32_t count, uint32_t* tid_out, int32_t* cnt, void* stream) {
    BMF_REQUIRE(tid_prev && x_t && pair && tid_out && cnt, "bmf_hyper_level: null pointer");
    BMF_REQUIRE(n_prev >= 1 && n >= 1 && ld_ok(ld), "bmf_hyper_level: need n_prev >= 1, n >= 1 and ld a multiple of 4 words, at most 2^26");
    BMF_REQUIRE(count_ok(count), "bmf_hyper_level: need 1 <= count <= 2^30 candidates");
    BMF_REQUIRE(bmf_aligned16(tid_prev) && bmf_aligned16(x_t) && bmf_aligned16(tid_out), "bmf_hyper_level: tid_prev, x_t and tid_out must be 16-byte aligned");
    BMF_REQUIRE(aligned4(pair) && aligned4(cnt), "bmf_hyper_level: pair and cnt must be 4-byte aligned");
    BMF_LAUNCH(hyper_level_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(tid_prev), n_prev,
               reinterpret_cast<const uint4*>(x_t), n, (int)(ld / 4), pair, count, reinterpret_cast<uint4*>(tid_out), cnt);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_hyper_eval(const uint32_t* tid, const uint32_t* rs_t, int32_t n, int64_t ld, const int32_t* items, int32_t maxlen,
                              const int32_t* ids, int32_t count, int32_t n_cand, uint32_t* T_out, int32_t* rec, void* stream) {
    BMF_REQUIRE(tid && rs_t && items && ids && T_out && rec, "bmf_hyper_eval: null pointer");
    BMF_REQUIRE(n >= 1 && ld_ok(ld), "bmf_hyper_eval: need n >= 1 and ld a multiple of 4 words, at most 2^26");
    BMF_REQUIRE(maxlen >= 1 && maxlen <= n, "bmf_hyper_eval: need 1 <= maxlen <= n columns per itemset");
    BMF_REQUIRE(count_ok(count) && count_ok(n_cand), "bmf_hyper_eval: need 1 <= count, n_cand <= 2^30 candidates");
    BMF_REQUIRE(bmf_aligned16(tid) && bmf_aligned16(rs_t) && bmf_aligned16(T_out), "bmf_hyper_eval: tid, rs_t and T_out must be 16-byte aligned");
    BMF_REQUIRE(aligned4(items) && aligned4(ids) && aligned4(rec), "bmf_hyper_eval: items, ids and rec must be 4-byte aligned");
    BMF_LAUNCH(hyper_eval_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(tid),
               reinterpret_cast<const uint4*>(rs_t), n, (int)(ld / 4), items, maxlen, ids, count, n_cand, reinterpret_cast<uint4*>(T_out), rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_hyper_copy(const uint32_t* src, int32_t n_src, const int32_t* src_id, uint32_t* dst, int32_t n_dst, const int32_t* dst_id,
                              int64_t ld, int32_t count, void* stream) {
    BMF_REQUIRE(src && src_id && dst && dst_id, "bmf_hyper_copy: null pointer");
    BMF_REQUIRE(src != dst, "bmf_hyper_copy: src and dst must be different arrays");
    BMF_REQUIRE(count_ok(n_src) && count_ok(n_dst) && ld_ok(ld), "bmf_hyper_copy: need 1 <= n_src, n_dst <= 2^30 and ld a multiple of 4 words, at most 2^26");
    BMF_REQUIRE(count_ok(count), "bmf_hyper_copy: need 1 <= count <= 2^30 rows");
    BMF_REQUIRE(bmf_aligned16(src) && bmf_aligned16(dst), "bmf_hyper_copy: src and dst must be 16-byte aligned");
    BMF_REQUIRE(aligned4(src_id) && aligned4(dst_id), "bmf_hyper_copy: src_id and dst_id must be 4-byte aligned");
    BMF_LAUNCH(hyper_copy_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(src), n_src, src_id,
               reinterpret_cast<uint4*>(dst), n_dst, dst_id, (int)(ld / 4), count);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
