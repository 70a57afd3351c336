// Concept search of GreConD on bit sets (PyBMF/models/GreConD.py:72-130), exact integer work.
//
// Everything reads the TRANSPOSED bit matrices: row c of Xt is column c of X as a bit row of W = m_pad / 32 words, so a set of rows of
// X (`u`) is one such bit row.  For a candidate column j and the row set best_u of the concept being grown:
//   u_j = Xt[j] & best_u,   v_j = { c : u_j is a subset of Xt[c] },   score_j = sum over c in v_j of |u_j & Xrs_t[c]|
//
// concept_scan_kernel   a workgroup holds the u_j of GROUP candidates in LDS; each of its waves takes columns c (every wave of every
//                       workgroup of the column split a different one), loads Xt[c] 64 words at a time (one word per lane) and tests the
//                       candidates still alive against them: one ballot of (u_j & ~Xt[c]) per candidate and chunk.  A column is left
//                       as soon as no candidate of the group can still contain it -- for a first sweep that is after the first chunk
//                       for nearly every column.  Survivors (c in v_j) add |u_j & Xrs_t[c]| to lane-local counters.
// concept_pick_kernel   adds the per-split partial sums in split order and finds the FIRST candidate of the list whose score exceeds
//                       best_score: the one record the host reads per launch.
// concept_close_*       best_u &= Xt[j] in place and best_v as a bit vector over the columns, for the accepted candidate only.
// concept_apply_*       Xrs_t[c] &= ~u, Xpd_t[c] |= u for c in v; then the residual count of every column and their sum (the sum, and
//                       the confusion counts of the prediction bits, are in bits_common.hip).
// Integer adds only, partial sums are added in a fixed order, no atomics: the same input gives the same output whatever the grid.
#include "bits_common.h"

#include <algorithm>

namespace {

constexpr int GROUP = 16;      // candidates per workgroup (their u_j share the LDS: GROUP * W words)
constexpr int WAVES = 4;       // waves per workgroup
constexpr int MAX_SPLIT = 64;  // column splits of one candidate group

// grid (groups of candidates, column splits), block 256.  LDS: GROUP * W words (dynamic) + the reduction scratch.
__global__ __launch_bounds__(256) void concept_scan_kernel(const uint32_t* __restrict__ Xt, const uint32_t* __restrict__ Xrs,
                                                           const uint32_t* __restrict__ best_u, const int32_t* __restrict__ cand,
                                                           int ncand, int n, int W, uint64_t* __restrict__ part_score,
                                                           uint32_t* __restrict__ part_nv, int32_t* __restrict__ out_nu) {
    extern __shared__ uint32_t u_lds[];                  // [GROUP][W]
    __shared__ uint64_t red_s[WAVES][GROUP];
    __shared__ uint32_t red_v[WAVES][GROUP], nu_s[GROUP];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int g0 = blockIdx.x * GROUP;
    const int ng = min(GROUP, ncand - g0);

    // u_j = Xt[j] & best_u into LDS, 16 threads per candidate; |u_j| on the way (written by the first column split)
    {
        const int q = t >> 4, r = t & 15;
        uint32_t cnt = 0;
        if (q < ng) {
            const uint32_t* xj = Xt + (int64_t)cand[g0 + q] * W;
            for (int w = r; w < W; w += 16) {
                const uint32_t x = xj[w] & best_u[w];
                u_lds[q * W + w] = x;
                cnt += __popc(x);
            }
        } else {
            for (int w = r; w < W; w += 16) u_lds[q * W + w] = 0;
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (r == 0) nu_s[q] = cnt;
        if (r == 0 && q < ng && blockIdx.y == 0) out_nu[g0 + q] = (int32_t)cnt;
    }
    __syncthreads();
    // an empty u_j lies in every column and covers nothing: |v_j| = n, score 0 without a test, so that such a candidate does not
    // keep its group from leaving a column early (late sweeps, where best_u is small, are full of them)
    uint32_t empty = 0;
#pragma unroll
    for (int j = 0; j < GROUP; ++j) empty |= (j < ng && nu_s[j] == 0u) ? 1u << j : 0u;

    uint32_t score[GROUP], nv[GROUP];   // score: lane-local; nv: the same in every lane
#pragma unroll
    for (int j = 0; j < GROUP; ++j) score[j] = nv[j] = 0;
    const uint32_t all = ((1u << ng) - 1u) & ~empty;
    const int nchunks = (W + 63) >> 6;

    const int c_first = blockIdx.y * WAVES + wave, c_step = gridDim.y * WAVES;
    for (int c = c_first; c < n; c += c_step) {
        const uint32_t* xc = Xt + (int64_t)c * W;
        uint32_t alive = all;
        for (int ch = 0; ch < nchunks && alive; ++ch) {
            const int w = ch * 64 + lane;
            const uint32_t notx = w < W ? ~xc[w] : 0u;
#pragma unroll
            for (int j = 0; j < GROUP; ++j) {
                if (alive >> j & 1u) {                   // (wave-uniform)
                    const uint32_t uj = w < W ? u_lds[j * W + w] : 0u;
                    if (__ballot((uj & notx) != 0u)) alive &= ~(1u << j);
                }
            }
            alive = (uint32_t)__builtin_amdgcn_readfirstlane((int)alive);   // (the same in every lane already: keep it scalar)
        }
        if (alive) {
            const uint32_t* rc = Xrs + (int64_t)c * W;
            for (int ch = 0; ch < nchunks; ++ch) {
                const int w = ch * 64 + lane;
                const uint32_t r = w < W ? rc[w] : 0u;
#pragma unroll
                for (int j = 0; j < GROUP; ++j)
                    if (alive >> j & 1u) score[j] += __popc((w < W ? u_lds[j * W + w] : 0u) & r);
            }
#pragma unroll
            for (int j = 0; j < GROUP; ++j) nv[j] += alive >> j & 1u;
        }
    }

    // lanes -> wave -> workgroup; one partial per (split, candidate).  A lane's score is at most ceil(W / 64) * 32 * n < 2^32 (checked
    // by the caller); 64 of them may not fit in 32 bits, so the halves are added apart and joined in 64 bits.
    const uint32_t my_cols = c_first < n ? (uint32_t)((n - c_first + c_step - 1) / c_step) : 0u;
#pragma unroll
    for (int j = 0; j < GROUP; ++j) {
        const uint32_t lo = wave_sum(score[j] & 0xffffu), hi = wave_sum(score[j] >> 16);
        if (lane == 0) {
            red_s[wave][j] = (uint64_t)lo + ((uint64_t)hi << 16);
            red_v[wave][j] = (empty >> j & 1u) ? my_cols : nv[j];
        }
    }
    __syncthreads();
    if (t < ng) {
        uint64_t s = 0;
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            s += red_s[w][t];
            v += red_v[w][t];
        }
        part_score[(int64_t)blockIdx.y * ncand + g0 + t] = s;
        part_nv[(int64_t)blockIdx.y * ncand + g0 + t] = v;
    }
}

// One block.  score / nv per candidate = the partials in split order; rec = { position of the first candidate with score >
// best_score or -1, its column or -1, its score, |u|, |v| } (zeros without a winner).
__global__ __launch_bounds__(256) void concept_pick_kernel(const uint64_t* __restrict__ part_score, const uint32_t* __restrict__ part_nv,
                                                           int splits, int ncand, const int32_t* __restrict__ cand,
                                                           const int32_t* __restrict__ nu, int64_t best_score,
                                                           int64_t* __restrict__ out_score, int32_t* __restrict__ out_nv,
                                                           int64_t* __restrict__ rec) {
    __shared__ int first[256];
    const int t = threadIdx.x;
    int mine = 0x7fffffff;
    for (int i = t; i < ncand; i += 256) {
        uint64_t s = 0;
        uint32_t v = 0;
        for (int p = 0; p < splits; ++p) {
            s += part_score[(int64_t)p * ncand + i];
            v += part_nv[(int64_t)p * ncand + i];
        }
        out_score[i] = (int64_t)s;
        out_nv[i] = (int32_t)v;
        if ((int64_t)s > best_score && i < mine) mine = i;
    }
    first[t] = mine;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) first[t] = min(first[t], first[t + o]);
        __syncthreads();
    }
    if (t == 0) {
        const int i = first[0];
        const bool hit = i != 0x7fffffff;
        rec[0] = hit ? i : -1;
        rec[1] = hit ? cand[i] : -1;
        rec[2] = hit ? out_score[i] : 0;   // (written by this thread's block before the barriers above)
        rec[3] = hit ? nu[i] : 0;
        rec[4] = hit ? out_nv[i] : 0;
    }
}

// best_u &= Xt[j].  j < 0: the column is rec[1]; nothing happens when that is -1.
__global__ __launch_bounds__(256) void concept_close_u_kernel(const uint32_t* __restrict__ Xt, int W, int j, const int64_t* __restrict__ rec,
                                                              uint32_t* __restrict__ best_u) {
    if (j < 0) j = (int)rec[1];
    if (j < 0) return;
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w < W) best_u[w] &= Xt[(int64_t)j * W + w];
}

// best_v: bit c = (best_u is a subset of Xt[c]), c < n; the bits of the padding columns are 0.  One thread per column, 64 columns per
// block; the subset test stops at the first word that fails.
__global__ __launch_bounds__(64) void concept_close_v_kernel(const uint32_t* __restrict__ Xt, int n, int W, int j, const int64_t* __restrict__ rec,
                                                             const uint32_t* __restrict__ best_u, uint32_t* __restrict__ best_v) {
    if (j < 0) j = (int)rec[1];
    if (j < 0) return;
    const int c = blockIdx.x * 64 + threadIdx.x;
    bool in = c < n;
    if (in) {
        const uint32_t* xc = Xt + (int64_t)c * W;
        for (int w = 0; w < W; ++w)
            if (best_u[w] & ~xc[w]) {
                in = false;
                break;
            }
    }
    const unsigned long long b = __ballot(in);
    if (threadIdx.x == 0) best_v[blockIdx.x * 2] = (uint32_t)b;
    if (threadIdx.x == 32) best_v[blockIdx.x * 2 + 1] = (uint32_t)(b >> 32);
}

// One wave per column, 4 columns per block: the column is changed when its bit of v is set; its residual count either way.
__global__ __launch_bounds__(256) void concept_apply_kernel(uint32_t* __restrict__ Xrs, uint32_t* __restrict__ Xpd, const uint32_t* __restrict__ u,
                                                            const uint32_t* __restrict__ v, int n, int W, int32_t* __restrict__ colcount) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n) return;
    const bool hit = v != nullptr && (v[c >> 5] >> (c & 31) & 1u);
    uint32_t* rc = Xrs + (int64_t)c * W;
    uint32_t* pc = Xpd + (int64_t)c * W;
    uint32_t cnt = 0;
    for (int w = lane; w < W; w += 64) {
        uint32_t r = rc[w];
        if (hit) {
            const uint32_t uw = u[w];
            r &= ~uw;
            rc[w] = r;
            pc[w] |= uw;
        }
        cnt += __popc(r);
    }
    cnt = wave_sum(cnt);
    if (lane == 0) colcount[c] = (int32_t)cnt;
}

int scan_splits(int ncand, int n) {
    const int groups = (ncand + GROUP - 1) / GROUP;
    int s = (4 * bmf_cu_count() + groups - 1) / groups;          // about four workgroups per compute unit
    s = std::min(s, (n + WAVES - 1) / WAVES);                     // a wave without a column has nothing to do
    return std::max(1, std::min(s, MAX_SPLIT));
}

}  // namespace

extern "C" int64_t bmf_concept_scan_work(int32_t ncand) {
    if (ncand < 1) return BMF_ERR_BAD_ARG;
    return (int64_t)MAX_SPLIT * ncand * 12;   // bytes: uint64 score + uint32 |v| per (split, candidate)
}

extern "C" int bmf_concept_scan(const uint32_t* Xt, const uint32_t* Xrs_t, int32_t n, int64_t ldw, const uint32_t* best_u,
                                const int32_t* cand, int32_t ncand, int64_t best_score, void* work, int64_t* score, int32_t* nu,
                                int32_t* nv, int64_t* rec, void* stream) {
    BMF_REQUIRE(Xt && Xrs_t && best_u && cand && work && score && nu && nv && rec, "bmf_concept_scan: null pointer");
    BMF_REQUIRE(n >= 1 && ncand >= 1 && ldw >= 1, "bmf_concept_scan: need n, ncand, ldw >= 1");
    // a choice, not the device's limit (160 KiB per workgroup): 64 KiB is what a launch gets without asking for more, and two
    // workgroups still share a compute unit
    BMF_REQUIRE(ldw * GROUP * 4 + 1024 <= 65536, "bmf_concept_scan: more than 32256 (padded) rows: the row sets of a candidate group and the reduction scratch are kept within 64 KiB of LDS");
    BMF_REQUIRE((int64_t)n * ((ldw + 63) / 64) * 32 < ((int64_t)1 << 32), "bmf_concept_scan: n * m_pad too large for the 32-bit lane counters");
    BMF_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0, "bmf_concept_scan: work must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int splits = scan_splits(ncand, n), groups = (ncand + GROUP - 1) / GROUP;
    uint64_t* part_score = static_cast<uint64_t*>(work);
    uint32_t* part_nv = reinterpret_cast<uint32_t*>(part_score + (int64_t)MAX_SPLIT * ncand);
    BMF_LAUNCH(concept_scan_kernel, dim3((unsigned)groups, (unsigned)splits), dim3(256), (size_t)(ldw * GROUP * 4), s, Xt, Xrs_t, best_u, cand,
               ncand, n, (int)ldw, part_score, part_nv, nu);
    BMF_LAUNCH(concept_pick_kernel, dim3(1), dim3(256), 0, s, part_score, part_nv, splits, ncand, cand, nu, best_score, score, nv, rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_concept_close(const uint32_t* Xt, int32_t n, int64_t ldw, int32_t j, const int64_t* rec, uint32_t* best_u,
                                 uint32_t* best_v, void* stream) {
    BMF_REQUIRE(Xt && best_u && best_v, "bmf_concept_close: null pointer");
    BMF_REQUIRE(n >= 1 && ldw >= 1 && j < n, "bmf_concept_close: need n, ldw >= 1 and j < n");
    BMF_REQUIRE(j >= 0 || rec, "bmf_concept_close: j < 0 takes the column from rec");
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(concept_close_u_kernel, dim3((unsigned)((ldw + 255) / 256)), dim3(256), 0, s, Xt, (int)ldw, j, rec, best_u);
    // best_v has ceil(n / 64) * 2 words
    BMF_LAUNCH(concept_close_v_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, Xt, n, (int)ldw, j, rec, best_u, best_v);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_concept_apply(uint32_t* Xrs_t, uint32_t* Xpd_t, int32_t n, int64_t ldw, const uint32_t* u, const uint32_t* v,
                                 int32_t* colcount, int64_t* rsum, void* stream) {
    BMF_REQUIRE(Xrs_t && Xpd_t && colcount && rsum, "bmf_concept_apply: null pointer");
    BMF_REQUIRE((u == nullptr) == (v == nullptr), "bmf_concept_apply: u and v come together (both null: only the counts)");
    BMF_REQUIRE(n >= 1 && ldw >= 1, "bmf_concept_apply: need n, ldw >= 1");
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(concept_apply_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, Xrs_t, Xpd_t, u, v, n, (int)ldw, colcount);
    bits_sum_launch(colcount, n, rsum, nullptr, s);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
