// Merge trials of Hyper+ on bit sets (PyBMF/models/HyperPlus.py:100-127, 169-185), exact integer work; every fp64 decision (the
// budget test fpb > beta, the savings and their comparison) is host arithmetic on the integers written here.
//
// Layouts are those of hyper.hip: x_t, pd_t are X and the cover transposed (bit row j = column j, ld = m_pad / 32 words); u_t holds the
// factors' T as k bit rows of ld words, v their I as k bit rows of ldv = n_pad / 32 words.  The merged rectangle T x I (T = T_a | T_b,
// I = I_a | I_b) contains both rectangles it replaces, so the cover of a trial is the current cover OR T x I, and the false positives
// it adds are the cells of T x I that are zero in X and not yet covered:
//   pairs   new_fp = sum_{j in I} |T & ~x_t[j] & ~pd_t[j]|,  |T|, |I|, |T_a & T_b|, |I_a & I_b|   per listed pair  (hyperplus_pairs_kernel)
//   union   u_t[dst] = u_t[a] | u_t[b],  v[dst] = v[a] | v[b]                                     the merge        (hyperplus_union_kernel)
// ~x & ~pd is all ones in the padding bits of a row: only the zero padding of T (of every u_t row) keeps them out of new_fp.
// One wave per pair, 4 per block: the lanes read 64 words of I at once and the wave takes the columns of the non-empty ones in turn;
// 16-byte loads along a row, one wave-level sum at the end.  No atomics: the same input gives the same output.
#include "bits_common.h"

namespace {

__device__ inline uint4 or4(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }

// 64-bit sum over the lanes of a wave from three 32-bit ones (bits 0-15, 16-31 and 32-57 of the lanes' totals: none can overflow)
__device__ inline int64_t wave_sum64(uint64_t v) {
    const uint64_t lo = wave_sum((unsigned)(v & 0xffffu)) + ((uint64_t)wave_sum((unsigned)((v >> 16) & 0xffffu)) << 16);
    return (int64_t)(lo + ((uint64_t)wave_sum((unsigned)(v >> 32)) << 32));
}

__global__ __launch_bounds__(256) void hyperplus_pairs_kernel(const uint4* __restrict__ u_t, const uint32_t* __restrict__ v, int k,
                                                              const uint4* __restrict__ x_t, const uint4* __restrict__ pd_t, int n, int ld4,
                                                              int ldv, const int32_t* __restrict__ pair, int count, int64_t* __restrict__ rec) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= count) return;
    const int a = pair[2 * c], b = pair[2 * c + 1];
    int64_t* out = rec + 5 * (int64_t)c;
    if (a < 0 || a >= k || b < 0 || b >= k || a == b) {                // (wave-uniform)
        if (lane < 5) out[lane] = -1;
        return;
    }
    const uint4 *ta = u_t + (int64_t)a * ld4, *tb = u_t + (int64_t)b * ld4;
    const uint32_t *ia = v + (int64_t)a * ldv, *ib = v + (int64_t)b * ldv;
    uint64_t fp = 0;
    uint32_t nI = 0, nIc = 0;
    const int nw = (n + 31) >> 5;                                      // the words of v that can hold a column < n
    for (int w0 = 0; w0 < nw; w0 += 64) {                              // 64 words of I at a time, one per lane
        const int w = w0 + lane;
        const uint32_t wa = w < nw ? ia[w] : 0u, wb = w < nw ? ib[w] : 0u, mine = wa | wb;
        nI += __popc(mine);
        nIc += __popc(wa & wb);
        for (uint64_t live = __ballot(mine != 0u); live; live &= live - 1) {              // the non-empty words, ascending (wave-uniform)
            const int src = __ffsll((unsigned long long)live) - 1;
            uint32_t bits = __builtin_amdgcn_readfirstlane(__shfl(mine, src, 64));
            for (; bits; bits &= bits - 1) {                           // its columns, one at a time (wave-uniform)
                const int j = 32 * (w0 + src) + __ffs(bits) - 1;
                if (j >= n) break;
                const uint4 *xj = x_t + (int64_t)j * ld4, *pj = pd_t + (int64_t)j * ld4;
                uint32_t s = 0;                                        // at most 2^26 * 32 / 64 = 2^25 bits per lane and column
#pragma unroll 2
                for (int q = lane; q < ld4; q += 64) s += popc4(andn4(or4(ta[q], tb[q]), or4(xj[q], pj[q])));
                fp += s;
            }
        }
    }
    uint32_t nT = 0, nTc = 0;
    for (int q = lane; q < ld4; q += 64) {
        const uint4 p = ta[q], r = tb[q];
        nT += popc4(or4(p, r));
        nTc += popc4(and4(p, r));
    }
    const int64_t fp_all = wave_sum64(fp);
    nT = wave_sum(nT);
    nTc = wave_sum(nTc);
    nI = wave_sum(nI);
    nIc = wave_sum(nIc);
    if (lane == 0) {
        out[0] = fp_all;
        out[1] = nT;
        out[2] = nI;
        out[3] = nTc;
        out[4] = nIc;
    }
}

// One block: the rows of T in uint4, then the words of I.  dst may be a or b (no __restrict__): a word is read and written by one lane.
__global__ __launch_bounds__(256) void hyperplus_union_kernel(uint4* u_t, uint32_t* v, int ld4, int ldv, int a, int b, int dst) {
    const uint4 *ta = u_t + (int64_t)a * ld4, *tb = u_t + (int64_t)b * ld4;
    uint4* td = u_t + (int64_t)dst * ld4;
    for (int q = threadIdx.x; q < ld4; q += 256) td[q] = or4(ta[q], tb[q]);
    const uint32_t *ia = v + (int64_t)a * ldv, *ib = v + (int64_t)b * ldv;
    uint32_t* id = v + (int64_t)dst * ldv;
    for (int w = threadIdx.x; w < ldv; w += 256) id[w] = ia[w] | ib[w];
}

inline bool id_ok(int32_t i, int32_t k) { return i >= 0 && i < k; }

}  // namespace

extern "C" int bmf_hyperplus_pairs(const uint32_t* u_t, const uint32_t* v, int32_t k, const uint32_t* x_t, const uint32_t* pd_t, int32_t n,
                                   int64_t ld, int64_t ldv, const int32_t* pair, int32_t count, int64_t* rec, void* stream) {
    BMF_REQUIRE(u_t && v && x_t && pd_t && pair && rec, "bmf_hyperplus_pairs: null pointer");
    BMF_REQUIRE(k >= 1 && n >= 1 && ld_ok(ld) && ld_ok(ldv), "bmf_hyperplus_pairs: need k >= 1, n >= 1 and ld, ldv multiples of 4 words, at most 2^26");
    BMF_REQUIRE((int64_t)n <= 32 * ldv, "bmf_hyperplus_pairs: need n <= 32 ldv columns");
    BMF_REQUIRE(count >= 1 && count <= (1 << 30), "bmf_hyperplus_pairs: need 1 <= count <= 2^30 pairs");
    BMF_REQUIRE(bmf_aligned16(u_t) && bmf_aligned16(v) && bmf_aligned16(x_t) && bmf_aligned16(pd_t),
                "bmf_hyperplus_pairs: u_t, v, x_t and pd_t must be 16-byte aligned");
    BMF_REQUIRE(aligned4(pair) && aligned8(rec), "bmf_hyperplus_pairs: pair must be 4-byte and rec 8-byte aligned");
    BMF_LAUNCH(hyperplus_pairs_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(u_t), v, k,
               reinterpret_cast<const uint4*>(x_t), reinterpret_cast<const uint4*>(pd_t), n, (int)(ld / 4), (int)ldv, pair, count, rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_hyperplus_union(uint32_t* u_t, uint32_t* v, int32_t k, int64_t ld, int64_t ldv, int32_t a, int32_t b, int32_t dst,
                                   void* stream) {
    BMF_REQUIRE(u_t && v, "bmf_hyperplus_union: null pointer");
    BMF_REQUIRE(k >= 1 && ld_ok(ld) && ld_ok(ldv), "bmf_hyperplus_union: need k >= 1 and ld, ldv multiples of 4 words, at most 2^26");
    BMF_REQUIRE(id_ok(a, k) && id_ok(b, k) && id_ok(dst, k), "bmf_hyperplus_union: a, b and dst must be factor ids in [0, k)");
    BMF_REQUIRE(bmf_aligned16(u_t) && bmf_aligned16(v), "bmf_hyperplus_union: u_t and v must be 16-byte aligned");
    BMF_LAUNCH(hyperplus_union_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<uint4*>(u_t), v, (int)(ld / 4), (int)ldv, a, b, dst);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
