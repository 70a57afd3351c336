// SimpleThreshold: the Boolean cover of EVERY pair (u_a, v_b) of a threshold grid in one chain of launches.
//
//   pd(a, b) = min(1, (U > u_a) @ (V > v_b)^T),  TP = sum(X o pd),  FP = sum(max(pd - X, 0))    (the counts of cover.hip, per pair)
//
// Two pieces:
//   * thresh_panels_kernel: the bits of an fp64 factor block under T threshold vectors, as the k-bit word of every row and as
//     bit-columns (the two layouts bmf_cover_count reads), strict F > thr in fp64;
//   * grid_cover_kernel: TP / FP of A row-word panels x B bit-column panels against the bits of X.
//
// The grid kernel uses that ascending thresholds give NESTED panels: a row's set factors only shrink as a grows.  A workgroup holds a
// chunk of CW words of the bit-columns of ONE panel b in LDS and a wave takes one row of X at a time (two words per lane, like
// cover_wide_kernel of wide.hip).  It walks the row's words from panel A - 1 down to panel 0: at step a only the factors that panel a
// adds to panel a + 1 are OR-ed in, and what they newly cover is counted -- d_tp(a) = |X & new|, d_p(a) = |new|.  A factor's
// bit-column is read once per (row, b), not once per (row, a, b), and a step that adds no factor costs a few scalar instructions.
// The counts of the pair are suffix sums, TP(a, b) = sum_{a' >= a} d_tp(a'), taken once per workgroup at the end.
//
// Where the per-step numbers go: the step index is wave-uniform but not a compile-time constant, so the accumulators cannot be
// registers, and a wave-wide integer reduction per step (six dependent cross-lane steps) would cost more than the step.  Each lane
// adds its two popcounts, packed as d_p << 16 | d_tp, to acc[a][lane] in LDS with one ds_add; a lane adds at most 64 per row and
// field, a workgroup takes at most 512 rows, so a field stays below 2^15 and never carries.  The workgroup unpacks and sums the 64
// lanes of each step, forms the suffix sums and adds them to the 64-bit counters: 2 A atomics per workgroup (cover.hip: one pair).
//
// The pair-list entry point runs the same kernel with one panel per "grid" (A = 1: a full walk of the row's word), so it assumes no
// nesting; the randomised search runs on it and the tests hold the grid walk to it.
// Two words per row (64 < k <= 128: two blocks per factor, blocks.py) is the template parameter NWORDS.
#include "common.h"

namespace {

constexpr int TG_CW = 128;       // words of a bit-column per workgroup: 64 lanes x 2 words
constexpr int TG_AMAX = 64;      // row-word panels per launch: one per lane of the load that fetches a row's words
constexpr int TG_RPB_MAX = 512;  // rows per workgroup: keeps the packed 16-bit fields of acc below 2^15
constexpr int TG_WAVES = 4;

__global__ __launch_bounds__(256) void thresh_panels_kernel(const double* __restrict__ F64, int64_t rows_pad, int rows, int k, int kp,
                                                             const double* __restrict__ thr, int T, uint64_t* __restrict__ rowbits,
                                                             uint32_t* __restrict__ colbits, int64_t ldcb) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // this wave's group of 64 rows
    if (gw * 64 >= rows_pad) return;
    const int64_t row = gw * 64 + lane;
    const bool live = row < rows;
    const double* fr = F64 + row * kp;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const double* th = thr + (int64_t)t * k;
        unsigned long long word = 0ull, mine = 0ull;
        for (int c = 0; c < k; ++c) {
            const bool bit = live && fr[c] > th[c];   // (padding rows are not read)
            const unsigned long long mask = __ballot(bit);
            word |= (unsigned long long)bit << c;
            if (lane == c) mine = mask;
        }
        if (rowbits) rowbits[(int64_t)t * rows_pad + row] = word;
        if (colbits && lane < kp)   // lane c holds the 64 rows of bit-column c (zero for k <= c < kp)
            *reinterpret_cast<u32x2*>(colbits + ((int64_t)t * kp + lane) * ldcb + gw * 2) = u32x2{(unsigned)mine, (unsigned)(mine >> 32)};
    }
}

// grid: (column chunks, row groups, panels b or pairs t).  PAIRS: pairs[z] names the two panels and the counters are counts[z][2].
template <int NWORDS, bool PAIRS>
__global__ __launch_bounds__(256) void grid_cover_kernel(const uint32_t* __restrict__ X, int64_t ldx, int64_t words, int64_t rows_pad,
                                                          int rows_per_block, const uint64_t* __restrict__ rb0,
                                                          const uint64_t* __restrict__ rb1, int A, int a0, int nA,
                                                          const uint32_t* __restrict__ cb0, const uint32_t* __restrict__ cb1, int64_t ldcb,
                                                          int kp, int B, int z0, const int32_t* __restrict__ pairs,
                                                          unsigned long long* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) uint32_t vt[NWORDS * 64][TG_CW];
    __shared__ unsigned acc[TG_AMAX][64];
    __shared__ unsigned tot[2][TG_AMAX];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int z = z0 + (int)blockIdx.z;
    int b = z;
    if (PAIRS) {
        a0 = pairs[2 * z];
        b = pairs[2 * z + 1];
        if (a0 < 0 || a0 >= A || b < 0 || b >= B) return;   // (uniform over the workgroup)
    }
    const int64_t w0 = (int64_t)blockIdx.x * TG_CW;
    const int nw = (int)min((int64_t)TG_CW, words - w0);   // a multiple of 4

    // LDS fill: the chunk of panel b's bit-columns, 16-byte pieces; columns >= kp and words >= nw are zero
    for (int p = threadIdx.x; p < NWORDS * 64 * (TG_CW / 4); p += 256) {
        const int l = p / (TG_CW / 4), pw = (p % (TG_CW / 4)) * 4;
        const int c = l & 63;
        const uint32_t* src = ((NWORDS == 2 && l >= 64) ? cb1 : cb0) + ((int64_t)b * kp + c) * ldcb + w0 + pw;
        *reinterpret_cast<u32x4*>(&vt[l][pw]) = (c < kp && pw < nw) ? *reinterpret_cast<const u32x4*>(src) : u32x4{0u, 0u, 0u, 0u};
    }
    for (int i = threadIdx.x; i < TG_AMAX * 64; i += 256) (&acc[0][0])[i] = 0u;
    __syncthreads();

    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = min(r0 + rows_per_block, rows_pad);
    const bool lane_on = 2 * lane < nw;
    const uint64_t* p0 = rb0 + (int64_t)(a0 + min(lane, nA - 1)) * rows_pad;   // lane a fetches the row's word of panel a0 + a
    const uint64_t* p1 = NWORDS == 2 ? rb1 + (int64_t)(a0 + min(lane, nA - 1)) * rows_pad : nullptr;
    for (int64_t r = r0 + wave; r < r1; r += TG_WAVES) {
        const unsigned long long w0v = lane < nA ? p0[r] : 0ull;
        const unsigned long long w1v = (NWORDS == 2 && lane < nA) ? p1[r] : 0ull;
        if (__ballot((w0v | w1v) != 0ull) == 0ull) continue;   // no panel sets a factor in this row
        const u32x2 x = lane_on ? *reinterpret_cast<const u32x2*>(X + r * ldx + w0 + 2 * lane) : u32x2{0u, 0u};
        const unsigned v00 = (unsigned)w0v, v01 = (unsigned)(w0v >> 32), v10 = (unsigned)w1v, v11 = (unsigned)(w1v >> 32);
        unsigned prev[4] = {0u, 0u, 0u, 0u};
        u32x2 pd = {0u, 0u};
        for (int a = nA - 1; a >= 0; --a) {
            unsigned add[4];
            add[0] = (unsigned)__builtin_amdgcn_readlane((int)v00, a) & ~prev[0];
            add[1] = (unsigned)__builtin_amdgcn_readlane((int)v01, a) & ~prev[1];
            add[2] = NWORDS == 2 ? (unsigned)__builtin_amdgcn_readlane((int)v10, a) & ~prev[2] : 0u;
            add[3] = NWORDS == 2 ? (unsigned)__builtin_amdgcn_readlane((int)v11, a) & ~prev[3] : 0u;
            if ((add[0] | add[1] | add[2] | add[3]) == 0u) continue;
            u32x2 nv = {0u, 0u};
#pragma unroll
            for (int q = 0; q < 2 * NWORDS; ++q) {
                unsigned w = add[q];
                prev[q] |= w;
                while (w) {
                    const int l = 32 * q + __builtin_ctz(w);
                    w &= w - 1;
                    nv |= *reinterpret_cast<const u32x2*>(&vt[l][2 * lane]);   // (lanes beyond the chunk read the zero fill)
                }
            }
            nv &= ~pd;   // what this step newly covers
            pd |= nv;
            const unsigned d = (unsigned)(__popc(x[0] & nv[0]) + __popc(x[1] & nv[1])) | ((unsigned)(__popc(nv[0]) + __popc(nv[1])) << 16);
            if (d) atomicAdd(&acc[a][lane], d);
        }
    }
    __syncthreads();
    // per step: the 64 lanes unpacked and summed (rotated start: no two threads on one bank), then the suffix sums over the steps
    if ((int)threadIdx.x < nA) {
        const int a = threadIdx.x;
        unsigned t = 0u, p = 0u;
        for (int j = 0; j < 64; ++j) {
            const unsigned v = acc[a][(j + a) & 63];
            t += v & 0xffffu;
            p += v >> 16;
        }
        tot[0][a] = t;
        tot[1][a] = p;
    }
    __syncthreads();
    if ((int)threadIdx.x < nA) {
        const int a = threadIdx.x;
        unsigned long long t = 0ull, p = 0ull;
        for (int j = a; j < nA; ++j) {
            t += tot[0][j];
            p += tot[1][j];
        }
        unsigned long long* out = PAIRS ? counts + 2 * (int64_t)z : counts + 2 * ((int64_t)(a0 + a) * B + b);
        if (t) atomicAdd(&out[0], t);
        if (p - t) atomicAdd(&out[1], p - t);   // FP = |P| - TP
    }
}

// rows per workgroup: the largest of 512 .. 64 that still leaves a thousand workgroups, else 64
int tg_rows_per_block(int64_t rows_pad, int64_t chunks, int64_t panels) {
    for (int rpb = TG_RPB_MAX; rpb > 64; rpb /= 2)
        if ((rows_pad + rpb - 1) / rpb * chunks * panels >= 1024) return rpb;
    return 64;
}

int tg_check(const char* who, const uint32_t* Xbits, int64_t rows_pad, int64_t ldx, int64_t words, const uint64_t* rowbits0,
             const uint64_t* rowbits1, int A, const uint32_t* colbits0, const uint32_t* colbits1, int64_t ldcb, int kp, int B,
             const unsigned long long* counts) {
    BMF_REQUIRE(Xbits && rowbits0 && colbits0 && counts, "%s: null pointer", who);
    BMF_REQUIRE((rowbits1 == nullptr) == (colbits1 == nullptr), "%s: rowbits1 and colbits1 go together (the second block of a rank above 64)", who);
    BMF_REQUIRE(rows_pad > 0 && rows_pad % 64 == 0 && rows_pad / 64 <= 65535, "%s: rows_pad must be a positive multiple of 64, at most 64 * 65535", who);
    BMF_REQUIRE(words > 0 && words % 4 == 0 && ldx >= words && ldx % 4 == 0, "%s: words/ldx must be multiples of 4, ldx >= words", who);
    BMF_REQUIRE(words <= (int64_t)TG_CW * 65535, "%s: words must be at most %d * 65535", who, TG_CW);
    BMF_REQUIRE(ldcb >= words && ldcb % 4 == 0, "%s: ldcb must be >= words and a multiple of 4", who);
    BMF_REQUIRE(kp == 32 || kp == 64, "%s: kp must be 32 or 64", who);
    BMF_REQUIRE(rowbits1 == nullptr || kp == 64, "%s: two blocks per factor need kp == 64", who);
    BMF_REQUIRE(A >= 1 && B >= 1 && B <= 65535, "%s: A must be >= 1 and B in 1..65535", who);
    BMF_REQUIRE(bmf_aligned16(Xbits) && bmf_aligned16(colbits0) && bmf_aligned16(colbits1), "%s: Xbits and colbits must be 16-byte aligned", who);
    return BMF_OK;
}

}  // namespace

extern "C" int bmf_thresh_panels(const double* F64, int64_t rows_pad, int32_t rows, int k, int kp, const double* thr, int T, uint64_t* rowbits,
                                 uint32_t* colbits, int64_t ldcb, void* stream) {
    BMF_REQUIRE(F64 && thr && (rowbits || colbits), "bmf_thresh_panels: null pointer");
    BMF_REQUIRE(rows_pad > 0 && rows_pad % 64 == 0, "bmf_thresh_panels: rows_pad must be a positive multiple of 64");
    BMF_REQUIRE(rows >= 1 && rows <= rows_pad, "bmf_thresh_panels: rows must be 1..rows_pad");
    BMF_REQUIRE(kp == 32 || kp == 64, "bmf_thresh_panels: kp must be 32 or 64");
    BMF_REQUIRE(k >= 1 && k <= kp, "bmf_thresh_panels: k=%d must be 1..kp", k);
    BMF_REQUIRE(T >= 1, "bmf_thresh_panels: T must be >= 1");
    BMF_REQUIRE(colbits == nullptr || (ldcb >= rows_pad / 32 && ldcb % 4 == 0), "bmf_thresh_panels: ldcb must be >= rows_pad / 32 and a multiple of 4");
    BMF_REQUIRE(bmf_aligned16(F64) && bmf_aligned16(colbits), "bmf_thresh_panels: F64 and colbits must be 16-byte aligned");
    const int64_t blocks = (rows_pad / 64 + 3) / 4;
    BMF_REQUIRE(blocks <= 0x7fffffff, "bmf_thresh_panels: rows_pad too large");
    BMF_LAUNCH(thresh_panels_kernel, dim3((unsigned)blocks, (unsigned)(T < 65535 ? T : 65535)), dim3(256), 0, (hipStream_t)stream, F64, rows_pad,
               rows, k, kp, thr, T, rowbits, colbits, ldcb);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_grid_cover_plan(int64_t rows_pad, int64_t words, int panels, int* chunk_words, int* rows_per_block, int* a_batch) {
    BMF_REQUIRE(chunk_words && rows_per_block && a_batch, "bmf_grid_cover_plan: null pointer");
    BMF_REQUIRE(rows_pad > 0 && rows_pad % 64 == 0 && words > 0 && words % 4 == 0 && panels >= 1, "bmf_grid_cover_plan: bad shape");
    *chunk_words = TG_CW;
    *rows_per_block = tg_rows_per_block(rows_pad, (words + TG_CW - 1) / TG_CW, panels);
    *a_batch = TG_AMAX;
    return BMF_OK;
}

extern "C" int bmf_grid_cover_count(const uint32_t* Xbits, int64_t rows_pad, int64_t ldx, int64_t words, const uint64_t* rowbits0,
                                    const uint64_t* rowbits1, int A, const uint32_t* colbits0, const uint32_t* colbits1, int64_t ldcb, int kp,
                                    int B, unsigned long long* counts, void* stream) {
    const int rc = tg_check("bmf_grid_cover_count", Xbits, rows_pad, ldx, words, rowbits0, rowbits1, A, colbits0, colbits1, ldcb, kp, B, counts);
    if (rc != BMF_OK) return rc;
    const int64_t chunks = (words + TG_CW - 1) / TG_CW;
    const int rpb = tg_rows_per_block(rows_pad, chunks, B);
    const dim3 grid((unsigned)chunks, (unsigned)((rows_pad + rpb - 1) / rpb), (unsigned)B);
    for (int a0 = 0; a0 < A; a0 += TG_AMAX) {   // each batch of panels is nested in itself: it starts its walk from nothing
        const int nA = A - a0 < TG_AMAX ? A - a0 : TG_AMAX;
        if (rowbits1)
            BMF_LAUNCH((grid_cover_kernel<2, false>), grid, dim3(256), 0, (hipStream_t)stream, Xbits, ldx, words, rows_pad, rpb, rowbits0, rowbits1, A,
                       a0, nA, colbits0, colbits1, ldcb, kp, B, 0, (const int32_t*)nullptr, counts);
        else
            BMF_LAUNCH((grid_cover_kernel<1, false>), grid, dim3(256), 0, (hipStream_t)stream, Xbits, ldx, words, rows_pad, rpb, rowbits0, rowbits1, A,
                       a0, nA, colbits0, colbits1, ldcb, kp, B, 0, (const int32_t*)nullptr, counts);
        BMF_LAUNCH_CHECK();
    }
    return BMF_OK;
}

extern "C" int bmf_pairs_cover_count(const uint32_t* Xbits, int64_t rows_pad, int64_t ldx, int64_t words, const uint64_t* rowbits0,
                                     const uint64_t* rowbits1, int A, const uint32_t* colbits0, const uint32_t* colbits1, int64_t ldcb, int kp,
                                     int B, const int32_t* pairs, int T, unsigned long long* counts, void* stream) {
    const int rc = tg_check("bmf_pairs_cover_count", Xbits, rows_pad, ldx, words, rowbits0, rowbits1, A, colbits0, colbits1, ldcb, kp, B, counts);
    if (rc != BMF_OK) return rc;
    BMF_REQUIRE(pairs && T >= 1, "bmf_pairs_cover_count: pairs must be given and T >= 1");
    const int64_t chunks = (words + TG_CW - 1) / TG_CW;
    const int rpb = tg_rows_per_block(rows_pad, chunks, T);
    for (int z0 = 0; z0 < T; z0 += 65535) {
        const int nz = T - z0 < 65535 ? T - z0 : 65535;
        const dim3 grid((unsigned)chunks, (unsigned)((rows_pad + rpb - 1) / rpb), (unsigned)nz);
        if (rowbits1)
            BMF_LAUNCH((grid_cover_kernel<2, true>), grid, dim3(256), 0, (hipStream_t)stream, Xbits, ldx, words, rows_pad, rpb, rowbits0, rowbits1, A, 0,
                       1, colbits0, colbits1, ldcb, kp, B, z0, pairs, counts);
        else
            BMF_LAUNCH((grid_cover_kernel<1, true>), grid, dim3(256), 0, (hipStream_t)stream, Xbits, ldx, words, rows_pad, rpb, rowbits0, rowbits1, A, 0,
                       1, colbits0, colbits1, ldcb, kp, B, z0, pairs, counts);
        BMF_LAUNCH_CHECK();
    }
    return BMF_OK;
}
