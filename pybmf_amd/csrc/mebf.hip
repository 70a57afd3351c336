// Median expansion of MEBF on bit sets (PyBMF/models/MEBF.py:112-231), exact integer work; the one fp64 decision is the reference's
// `count > t * |a|`.
//
// A growth along one axis only touches the bit matrices of ONE orientation: N bit rows of ld words, zero padded.  Axis 0 takes the
// transposed matrices (bit row j = column j of X, ld = m_pad / 32), axis 1 the row-major ones.  With rs the residual, x the data and
// pd the cover in that orientation:
//   score_j = |rs_j|                          (bmf_mebf_scores, bits_common.hip; refreshed by apply for the rows it changed)
//   mid     = the index at rank P / 2 of the P positive scores under (score descending, index descending)      (mebf_select_kernel)
//   a       = rs_mid, or rs_first & rs_second for the weak signal                                             (mebf_take_a_kernel)
//   c_j     = |rs_j & a|,  b_j = (double)c_j > t * (double)|a|,  and for the rows of b only
//   tp_j    = |a & x_j & ~pd_j|,  fp_j = |a & ~x_j & ~pd_j|                                                    (mebf_grow_kernel)
//   b as bits, |a|, |b|, dTP = sum tp_j, dFP = sum fp_j                                                        (mebf_finish_kernel)
// rs, x and pd are three arguments because a fit that truncated a factor grows on the residual it has while it counts against the
// cover of the factors it kept; otherwise x & ~pd = rs and dTP = sum of c_j over b.
// mebf_apply_kernel: for the bit rows named by `hit`: rs_j &= ~mask, pd_j |= mask, and their new |rs_j|, |pd_j|.
// Integer adds in a fixed order, no atomics: the same input gives the same output whatever the grid.
#include "bits_common.h"

namespace {

constexpr int SEL_THREADS = 1024;

// the block's sum / maximum of v, the same in every thread (red: 16 ints of LDS)
__device__ inline int block_sum(int v, int* red) {
    v = (int)wave_sum((uint32_t)v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

__device__ inline int block_max(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = red[0];
#pragma unroll
    for (int w = 1; w < SEL_THREADS / 64; ++w) s = max(s, red[w]);
    __syncthreads();
    return s;
}

// The index at `rank` (0-based, rank < N) of the order (score descending, index descending).  Bisection on the score value at the
// rank (at most 32 counting passes over the vector), then one counting pass over the indices of that tie group: every thread owns a
// contiguous chunk of indices, thread 0 walks the 1024 chunk counts from the top, the owner walks its chunk.  Whole block.
__device__ int select_rank(const int32_t* __restrict__ score, int N, int rank, int mx, int* red, int* cnt, int* pick) {
    const int t = threadIdx.x;
    int lo = 0, hi = mx;                      // the largest value T with |{score >= T}| >= rank + 1
    while (lo < hi) {
        const int T = lo + (hi - lo + 1) / 2;
        int c = 0;
        for (int i = t; i < N; i += SEL_THREADS) c += score[i] >= T;
        if (block_sum(c, red) >= rank + 1) lo = T; else hi = T - 1;
    }
    const int s = lo;
    int above = 0;
    for (int i = t; i < N; i += SEL_THREADS) above += score[i] > s;
    const int r = rank - block_sum(above, red);   // the position inside the tie group, counted from its highest index
    const int chunk = (N + SEL_THREADS - 1) / SEL_THREADS;
    const int i0 = min(N, t * chunk), i1 = min(N, i0 + chunk);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += score[i] == s;
    cnt[t] = mine;
    __syncthreads();
    if (t == 0) {
        int left = r, owner = -1;
        for (int q = SEL_THREADS - 1; q >= 0; --q) {
            if (left < cnt[q]) {
                owner = q;
                break;
            }
            left -= cnt[q];
        }
        pick[0] = owner;
        pick[1] = left;
    }
    __syncthreads();
    if (t == pick[0]) {
        int left = pick[1];
        for (int i = i1 - 1; i >= i0; --i)
            if (score[i] == s && left-- == 0) {
                pick[2] = i;
                break;
            }
    }
    __syncthreads();
    const int found = pick[2];
    __syncthreads();
    return found;
}

// One block.  weak == 0: rec[0] = the median index of the P positive scores (-1 when P = 0), rec[1] = P.
// weak != 0: rec[0], rec[1] = the indices at ranks 0 and 1 of all N >= 2 scores.  rec[2..7] = 0.
__global__ __launch_bounds__(SEL_THREADS) void mebf_select_kernel(const int32_t* __restrict__ score, int N, int weak, int64_t* __restrict__ rec) {
    __shared__ int red[SEL_THREADS / 64], cnt[SEL_THREADS], pick[3];
    const int t = threadIdx.x;
    int p = 0, m = 0;
    for (int i = t; i < N; i += SEL_THREADS) {
        p += score[i] > 0;
        m = max(m, score[i]);
    }
    const int P = block_sum(p, red), mx = block_max(m, red);
    int first, second;
    if (weak) {
        first = select_rank(score, N, 0, mx, red, cnt, pick);
        second = select_rank(score, N, 1, mx, red, cnt, pick);
    } else {
        first = P > 0 ? select_rank(score, N, P / 2, mx, red, cnt, pick) : -1;   // (P is the same in every thread)
        second = P;
    }
    if (t < 8) rec[t] = t == 0 ? first : t == 1 ? second : 0;
}

// a = rs[rec[0]] (weak: & rs[rec[1]]), ld words; all zero when rec[0] < 0.
__global__ __launch_bounds__(256) void mebf_take_a_kernel(const uint32_t* __restrict__ rs, int ld, const int64_t* __restrict__ rec, int weak,
                                                          uint32_t* __restrict__ a) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= ld) return;
    const int64_t i0 = rec[0], i1 = weak ? rec[1] : rec[0];
    a[w] = i0 < 0 ? 0u : rs[i0 * ld + w] & rs[i1 * ld + w];
}

// One wave per bit row, 4 rows per block, 16-byte loads (a lane takes every 64th uint4 of the row: 1 KiB per wave and load).
// cnt[j] = |rs_j & a|; for the rows with (double)cnt > t * |a| also tp[j], fp[j].  |a| is counted on the way by every wave.
__global__ __launch_bounds__(256) void mebf_grow_kernel(const uint4* __restrict__ rs, const uint4* __restrict__ x, const uint4* __restrict__ pd,
                                                        int N, int ld4, const uint4* __restrict__ a, double t, int32_t* __restrict__ cnt,
                                                        int32_t* __restrict__ tp, int32_t* __restrict__ fp) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= N) return;
    const int64_t base = (int64_t)j * ld4;
    uint32_t c = 0, na = 0;
#pragma unroll 2
    for (int w = lane; w < ld4; w += 64) {
        const uint4 av = a[w];
        c += popc4(and4(rs[base + w], av));
        na += popc4(av);
    }
    c = wave_sum(c);
    na = wave_sum(na);
    const bool in = (double)c > t * (double)na;          // (wave-uniform)
    uint32_t p = 0, q = 0;
    if (in) {
#pragma unroll 2
        for (int w = lane; w < ld4; w += 64) {
            const uint4 free_a = andn4(a[w], pd[base + w]), xv = x[base + w];
            p += popc4(and4(free_a, xv));
            q += popc4(andn4(free_a, xv));
        }
        p = wave_sum(p);
        q = wave_sum(q);
    }
    if (lane == 0) {
        cnt[j] = (int32_t)c;
        tp[j] = (int32_t)p;
        fp[j] = (int32_t)q;
    }
}

// One block: b (nbw words, bits >= N zero), rec[2..5] = |a|, |b|, dTP, dFP.
__global__ __launch_bounds__(256) void mebf_finish_kernel(const uint32_t* __restrict__ a, int ld, double t, const int32_t* __restrict__ cnt,
                                                          const int32_t* __restrict__ tp, const int32_t* __restrict__ fp, int N, int nbw,
                                                          uint32_t* __restrict__ b, int64_t* __restrict__ rec) {
    __shared__ int64_t red[3][256];
    __shared__ uint32_t na_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t na = 0;
    for (int w = tid; w < ld; w += 256) na += __popc(a[w]);
    red[0][tid] = na;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[0][tid] += red[0][tid + o];
        __syncthreads();
    }
    if (tid == 0) na_s = (uint32_t)red[0][0];
    __syncthreads();
    const double thr = t * (double)na_s;
    int64_t nb = 0, stp = 0, sfp = 0;
    for (int j0 = 0; j0 < nbw * 32; j0 += 256) {
        const int j = j0 + tid;
        const bool in = j < N && (double)cnt[j] > thr;
        if (in) {
            nb += 1;
            stp += tp[j];
            sfp += fp[j];
        }
        const unsigned long long bits = __ballot(in);
        const int word = (j0 >> 5) + wave * 2;
        if (lane == 0 && word < nbw) b[word] = (uint32_t)bits;
        if (lane == 32 && word + 1 < nbw) b[word + 1] = (uint32_t)(bits >> 32);
    }
    __syncthreads();
    red[0][tid] = nb;
    red[1][tid] = stp;
    red[2][tid] = sfp;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
            red[2][tid] += red[2][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        rec[2] = na_s;
        rec[3] = red[0][0];
        rec[4] = red[1][0];
        rec[5] = red[2][0];
    }
}

// One wave per bit row, 4 rows per block; only the rows whose bit of `hit` is set are read and written.
__global__ __launch_bounds__(256) void mebf_apply_kernel(uint32_t* __restrict__ rs, uint32_t* __restrict__ pd, int N, int ld,
                                                         const uint32_t* __restrict__ hit, const uint32_t* __restrict__ mask,
                                                         int32_t* __restrict__ score, int32_t* __restrict__ pdcount) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= N || !(hit[j >> 5] >> (j & 31) & 1u)) return;
    uint32_t* r = rs + (int64_t)j * ld;
    uint32_t* p = pd + (int64_t)j * ld;
    uint32_t cr = 0, cp = 0;
    for (int w = lane; w < ld; w += 64) {
        const uint32_t mw = mask[w], rv = r[w] & ~mw, pv = p[w] | mw;
        r[w] = rv;
        p[w] = pv;
        cr += __popc(rv);
        cp += __popc(pv);
    }
    cr = wave_sum(cr);
    cp = wave_sum(cp);
    if (lane == 0) {
        score[j] = (int32_t)cr;
        pdcount[j] = (int32_t)cp;
    }
}

}  // namespace

extern "C" int bmf_mebf_select(const int32_t* score, int32_t N, int32_t weak, int64_t* rec, void* stream) {
    BMF_REQUIRE(score && rec, "bmf_mebf_select: null pointer");
    BMF_REQUIRE(N >= 1, "bmf_mebf_select: need N >= 1");
    BMF_REQUIRE(!weak || N >= 2, "bmf_mebf_select: the weak signal takes the two highest of at least 2 scores");
    BMF_LAUNCH(mebf_select_kernel, dim3(1), dim3(SEL_THREADS), 0, (hipStream_t)stream, score, N, weak, rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_mebf_weak_a(const uint32_t* rs, int64_t ld, const int64_t* rec, uint32_t* a, void* stream) {
    BMF_REQUIRE(rs && rec && a, "bmf_mebf_weak_a: null pointer");
    BMF_REQUIRE(ld >= 1 && ld <= (1 << 26), "bmf_mebf_weak_a: need 1 <= ld <= 2^26");
    BMF_LAUNCH(mebf_take_a_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rs, (int)ld, rec, 1, a);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int64_t bmf_mebf_grow_work(int32_t N) {
    if (N < 1) return BMF_ERR_BAD_ARG;
    return (int64_t)N * 12;   // bytes: int32 count, tp, fp per bit row
}

extern "C" int bmf_mebf_grow(const uint32_t* rs, const uint32_t* x, const uint32_t* pd, int32_t N, int64_t ld, uint32_t* a,
                             int32_t a_from_rec, double t, void* work, uint32_t* b, int32_t nbw, int64_t* rec, void* stream) {
    BMF_REQUIRE(rs && x && pd && a && work && b && rec, "bmf_mebf_grow: null pointer");
    BMF_REQUIRE(N >= 1 && ld_ok(ld), "bmf_mebf_grow: need N >= 1 and ld a multiple of 4 words, at most 2^26");
    BMF_REQUIRE((int64_t)nbw * 32 >= N, "bmf_mebf_grow: b needs at least ceil(N / 32) words");
    BMF_REQUIRE(bmf_aligned16(rs) && bmf_aligned16(x) && bmf_aligned16(pd) && bmf_aligned16(a), "bmf_mebf_grow: rs, x, pd and a must be 16-byte aligned");
    BMF_REQUIRE((reinterpret_cast<uintptr_t>(work) & 3u) == 0, "bmf_mebf_grow: work must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    int32_t* cnt = static_cast<int32_t*>(work);
    int32_t *tp = cnt + N, *fp = cnt + 2 * (int64_t)N;
    if (a_from_rec) BMF_LAUNCH(mebf_take_a_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, s, rs, (int)ld, rec, 0, a);
    BMF_LAUNCH(mebf_grow_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const uint4*>(rs), reinterpret_cast<const uint4*>(x),
               reinterpret_cast<const uint4*>(pd), N, (int)(ld / 4), reinterpret_cast<const uint4*>(a), t, cnt, tp, fp);
    BMF_LAUNCH(mebf_finish_kernel, dim3(1), dim3(256), 0, s, a, (int)ld, t, cnt, tp, fp, N, nbw, b, rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_mebf_apply(uint32_t* rs, uint32_t* pd, int32_t N, int64_t ld, const uint32_t* hit, const uint32_t* mask, int32_t* score,
                              int32_t* pdcount, int64_t* out, void* stream) {
    BMF_REQUIRE(rs && pd && hit && mask && score && pdcount && out, "bmf_mebf_apply: null pointer");
    BMF_REQUIRE(N >= 1 && ld >= 1 && ld <= (1 << 26), "bmf_mebf_apply: need N >= 1 and 1 <= ld <= 2^26");
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(mebf_apply_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, rs, pd, N, (int)ld, hit, mask, score, pdcount);
    bits_sum_launch(score, N, out, nullptr, s);
    bits_sum_launch(pdcount, N, out + 1, nullptr, s);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
