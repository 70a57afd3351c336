// Asso (PyBMF/models/Asso.py): candidate basis rows from the column associations, and the scoring of every candidate against the
// current prediction as two AND-popcount contractions with an fp64 epilogue.  Exact integers; partial sums are added in a fixed
// order; no atomics: the same input gives the same bytes whatever the grid.
//
// Row-major bit matrices throughout, `ldx` = n_pad / 32 words per row (a multiple of 16): X, the prediction PD, and the candidate
// matrix B (row i = basis vector of column i); only asso_basis_kernel reads the TRANSPOSED bits of X (one row of ldw = m_pad / 32
// words per column).
//
// asso_basis_kernel    64 x 64 tile of C = X^T X per workgroup, rows of X^T staged in LDS 32 words at a time, a 4 x 4 register tile of
//                      popcount sums per thread; then bit (i, j) = C[i][j] / C[i][i] > tau in fp64, written as packed words.  C is
//                      never stored.  The bits of every row are then counted (bits_common.hip: an empty row is no candidate).
// asso_score_kernel    64 rows of X x 64 candidates per workgroup.  Per row r and candidate b:
//                        a = |x_r & ~pd_r & b|,  a + c = |~pd_r & b|;   TP_new = TP_old + a,  FP_new = FP_old + c
//                      ~pd_r and x_r & ~pd_r are formed once while the row tile is staged; both operands sit in LDS 16 words at a time
//                      (double buffered), every thread keeps a 4 x 4 tile of (a, a + c) in registers.  The epilogue decides per (r, b)
//                      whether row r takes the candidate:  -w_fp FP_new + w_fn TP_new > -w_fp FP_old + w_fn TP_old, in fp64 with two
//                      products and one sum per side as the reference writes it (no contraction), adds the chosen TP / FP over the
//                      tile's rows and writes one (T, F) pair per (row tile, candidate).
// asso_reduce_kernel   adds the pairs in row-tile order, one thread per candidate: T, F and score = w_fn T - w_fp F.
// asso_pick_kernel     records the candidate with the largest score above best_score, the first of equals -- what the reference's
//                      sweep keeps.
// asso_column_kernel   the same per-row decision for one candidate, written as the bits of u, and |u|.
// asso_apply_kernel    PD_r |= v for the rows r of u.
#include "bits_common.h"

namespace {

constexpr int TILE = 64;        // rows and candidates per workgroup of the score kernel
constexpr int KW = 16;          // words per LDS stage
constexpr int LDW = KW + 4;     // LDS row stride in words: 16 rows 20 words apart fall into 16 different groups of 4 banks
constexpr int BKW = 32;         // words per LDS stage of the basis kernel
constexpr int BLD = BKW + 4;

// the reference's row score, exactly as it is written there: (-w_fp) * FP + w_fn * TP
__device__ __forceinline__ double row_score(double w_fp, double w_fn, uint32_t tp, uint32_t fp) {
    return __dadd_rn(__dmul_rn(-w_fp, (double)fp), __dmul_rn(w_fn, (double)tp));
}

// grid (ceil(n / 64), ceil(n / 64)): x = tile of j (bits), y = tile of i (rows of B).  block 256.
__global__ __launch_bounds__(256) void asso_basis_kernel(const uint32_t* __restrict__ Xt, int n, int W, double tau,
                                                         uint32_t* __restrict__ B, int ldb) {
    __shared__ __attribute__((aligned(16))) uint32_t sa[TILE * BLD], sb[TILE * BLD];
    __shared__ uint32_t diag[TILE];
    __shared__ uint8_t flag[TILE][TILE + 4];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
    const int lr = t >> 2, lw = (t & 3) * 8;          // this thread stages 8 words of row lr of both tiles
    const bool ia = i0 + lr < n, ja = j0 + lr < n;    // (rows >= n are not read: treated as empty)
    const uint32_t* pa = Xt + (int64_t)(i0 + lr) * W + lw;
    const uint32_t* pb = Xt + (int64_t)(j0 + lr) * W + lw;
    uint32_t acc[4][4] = {};
    uint32_t mine = 0;                                // popcount of row i0 + lr over this thread's words: C[i][i]
    for (int w0 = 0; w0 < W; w0 += BKW) {
        u32x4 a0 = {0, 0, 0, 0}, a1 = a0, b0 = a0, b1 = a0;
        if (w0 + lw < W) {                            // W is a multiple of 16, lw of 8: 8 words are in or out together
            if (ia) {
                a0 = *reinterpret_cast<const u32x4*>(pa + w0);
                a1 = *reinterpret_cast<const u32x4*>(pa + w0 + 4);
            }
            if (ja) {
                b0 = *reinterpret_cast<const u32x4*>(pb + w0);
                b1 = *reinterpret_cast<const u32x4*>(pb + w0 + 4);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) mine += __popc(a0[q]) + __popc(a1[q]);
        __syncthreads();
        *reinterpret_cast<u32x4*>(&sa[lr * BLD + lw]) = a0;
        *reinterpret_cast<u32x4*>(&sa[lr * BLD + lw + 4]) = a1;
        *reinterpret_cast<u32x4*>(&sb[lr * BLD + lw]) = b0;
        *reinterpret_cast<u32x4*>(&sb[lr * BLD + lw + 4]) = b1;
        __syncthreads();
#pragma unroll 2
        for (int w = 0; w < BKW; w += 4) {
            u32x4 ra[4], rb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) ra[a] = *reinterpret_cast<const u32x4*>(&sa[(ty + 16 * a) * BLD + w]);
#pragma unroll
            for (int b = 0; b < 4; ++b) rb[b] = *reinterpret_cast<const u32x4*>(&sb[(tx + 16 * b) * BLD + w]);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[a][b] += __popc(ra[a][q] & rb[b][q]);
        }
    }
    mine += __shfl_xor(mine, 1);
    mine += __shfl_xor(mine, 2);
    if ((t & 3) == 0) diag[lr] = mine;
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int li = ty + 16 * a;
        const uint32_t s = diag[li];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int lj = tx + 16 * b;
            // assoc = C / s in fp64 (IEEE division), 0 for an empty column; basis = assoc > tau, strict
            const bool on = s > 0u && i0 + li < n && j0 + lj < n && (double)acc[a][b] / (double)s > tau;
            flag[li][lj] = on ? 1 : 0;
        }
    }
    __syncthreads();
    if (t < 2 * TILE) {
        const int li = t >> 1, h = t & 1;
        uint32_t word = 0;
#pragma unroll
        for (int q = 0; q < 32; ++q) word |= (uint32_t)flag[li][32 * h + q] << q;
        if (i0 + li < n) B[(int64_t)(i0 + li) * ldb + (j0 >> 5) + h] = word;   // (j0 / 32 + h < ldb: n_pad is a multiple of 64)
    }
}

// grid (ceil(ncand / 64), ceil(m / 64)), block 256 = 16 (tx: candidates tx + 16 b) x 16 (ty: rows ty + 16 a).
__global__ __launch_bounds__(256) void asso_score_kernel(const uint32_t* __restrict__ X, const uint32_t* __restrict__ PD,
                                                         const uint32_t* __restrict__ B, int ldx, int m, int n_rows_b,
                                                         const int32_t* __restrict__ cand, int ncand,
                                                         const uint32_t* __restrict__ tp_old, const uint32_t* __restrict__ fp_old,
                                                         double w_fp, double w_fn, int64_t* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) uint32_t s_xn[2][TILE * LDW], s_np[2][TILE * LDW], s_b[2][TILE * LDW];
    __shared__ uint32_t red_t[16][TILE], red_f[16][TILE];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int r0 = blockIdx.y * TILE, c0 = blockIdx.x * TILE;
    const int lr = t >> 2, lw = (t & 3) * 4;          // this thread stages 4 words of row lr of the three tiles
    // a row past m is not read (it is left out of the sums below); a candidate slot past the list, or an index outside B, reads as empty
    const bool row_in = r0 + lr < m;
    const uint32_t* px = X + (int64_t)(row_in ? r0 + lr : 0) * ldx + lw;
    const uint32_t* pp = PD + (int64_t)(row_in ? r0 + lr : 0) * ldx + lw;
    const int cj = c0 + lr < ncand ? cand[c0 + lr] : -1;
    const bool cb_in = cj >= 0 && cj < n_rows_b;
    const uint32_t* pb = B + (int64_t)(cb_in ? cj : 0) * ldx + lw;
    const u32x4 zero = {0, 0, 0, 0};

    uint32_t acc_a[4][4] = {}, acc_n[4][4] = {};      // a and a + c
    u32x4 gx = *reinterpret_cast<const u32x4*>(px), gp = *reinterpret_cast<const u32x4*>(pp);
    u32x4 gb = cb_in ? *reinterpret_cast<const u32x4*>(pb) : zero;
    {
        const u32x4 np = ~gp;
        *reinterpret_cast<u32x4*>(&s_np[0][lr * LDW + lw]) = np;
        *reinterpret_cast<u32x4*>(&s_xn[0][lr * LDW + lw]) = gx & np;
        *reinterpret_cast<u32x4*>(&s_b[0][lr * LDW + lw]) = gb;
    }
    __syncthreads();
    const int stages = ldx / KW;
    for (int st = 0; st < stages; ++st) {
        const int cur = st & 1;
        if (st + 1 < stages) {                        // the next stage's words travel while this one is counted
            gx = *reinterpret_cast<const u32x4*>(px + (st + 1) * KW);
            gp = *reinterpret_cast<const u32x4*>(pp + (st + 1) * KW);
            gb = cb_in ? *reinterpret_cast<const u32x4*>(pb + (st + 1) * KW) : zero;
        }
#pragma unroll 1   // (one step's operands are 48 registers; unrolled, the four steps' loads are hoisted and the kernel needs 256)
        for (int w = 0; w < KW; w += 4) {
            u32x4 rx[4], rn[4], rb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                rx[a] = *reinterpret_cast<const u32x4*>(&s_xn[cur][(ty + 16 * a) * LDW + w]);
                rn[a] = *reinterpret_cast<const u32x4*>(&s_np[cur][(ty + 16 * a) * LDW + w]);
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) rb[b] = *reinterpret_cast<const u32x4*>(&s_b[cur][(tx + 16 * b) * LDW + w]);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        acc_a[a][b] += __popc(rx[a][q] & rb[b][q]);
                        acc_n[a][b] += __popc(rn[a][q] & rb[b][q]);
                    }
        }
        if (st + 1 < stages) {
            const u32x4 np = ~gp;
            *reinterpret_cast<u32x4*>(&s_np[cur ^ 1][lr * LDW + lw]) = np;
            *reinterpret_cast<u32x4*>(&s_xn[cur ^ 1][lr * LDW + lw]) = gx & np;
            *reinterpret_cast<u32x4*>(&s_b[cur ^ 1][lr * LDW + lw]) = gb;
        }
        __syncthreads();   // the other buffer is full, and nobody reads this one any more
    }

    // per (row, candidate): does the row take the candidate?  Then the chosen TP / FP, added over this thread's four rows
    uint32_t sum_t[4] = {}, sum_f[4] = {};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int r = r0 + ty + 16 * a;
        if (r < m) {
            const uint32_t tpo = tp_old[r], fpo = fp_old[r];
            const double s_old = row_score(w_fp, w_fn, tpo, fpo);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t tpn = tpo + acc_a[a][b], fpn = fpo + (acc_n[a][b] - acc_a[a][b]);
                const bool take = row_score(w_fp, w_fn, tpn, fpn) > s_old;
                sum_t[b] += take ? tpn : tpo;
                sum_f[b] += take ? fpn : fpo;
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        red_t[ty][tx + 16 * b] = sum_t[b];
        red_f[ty][tx + 16 * b] = sum_f[b];
    }
    __syncthreads();
    if (t < TILE && c0 + t < ncand) {
        int64_t T = 0, F = 0;
#pragma unroll
        for (int y = 0; y < 16; ++y) {
            T += red_t[y][t];
            F += red_f[y][t];
        }
        int64_t* out = part + ((int64_t)blockIdx.y * ncand + c0 + t) * 2;
        out[0] = T;
        out[1] = F;
    }
}

// One thread per candidate: T, F = the pairs of the row tiles added in tile order (neighbouring threads read neighbouring pairs),
// score = w_fn T - w_fp F.
__global__ __launch_bounds__(256) void asso_reduce_kernel(const int64_t* __restrict__ part, int tiles, int ncand, double w_fp, double w_fn,
                                                          int64_t* __restrict__ out_t, int64_t* __restrict__ out_f,
                                                          double* __restrict__ out_score) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ncand) return;
    int64_t T = 0, F = 0;
    for (int p = 0; p < tiles; ++p) {
        T += part[((int64_t)p * ncand + i) * 2];
        F += part[((int64_t)p * ncand + i) * 2 + 1];
    }
    out_t[i] = T;
    out_f[i] = F;
    out_score[i] = __dsub_rn(__dmul_rn(w_fn, (double)T), __dmul_rn(w_fp, (double)F));
}

// One block.  rec = { position, candidate, score (the bits of the double), T, F } of the largest score above best_score, the first of
// equals, or { -1, -1, bits of best_score, 0, 0 }.
__global__ __launch_bounds__(256) void asso_pick_kernel(const int64_t* __restrict__ out_t, const int64_t* __restrict__ out_f,
                                                        const double* __restrict__ out_score, int ncand, const int32_t* __restrict__ cand,
                                                        double best_score, int64_t* __restrict__ rec) {
    __shared__ double top_s[256];
    __shared__ int top_i[256];
    const int t = threadIdx.x;
    double best = best_score;
    int at = 0x7fffffff;
    for (int i = t; i < ncand; i += 256) {
        const double s = out_score[i];
        if (s > best) {           // (ascending i: an equal later score does not replace)
            best = s;
            at = i;
        }
    }
    top_s[t] = best;
    top_i[t] = at;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            const double s2 = top_s[t + o];
            const int i2 = top_i[t + o];
            if (i2 != 0x7fffffff && (top_i[t] == 0x7fffffff || s2 > top_s[t] || (s2 == top_s[t] && i2 < top_i[t]))) {
                top_s[t] = s2;
                top_i[t] = i2;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        const int i = top_i[0];
        const bool hit = i != 0x7fffffff;
        rec[0] = hit ? i : -1;
        rec[1] = hit ? cand[i] : -1;
        rec[2] = __double_as_longlong(hit ? top_s[0] : best_score);
        rec[3] = hit ? out_t[i] : 0;
        rec[4] = hit ? out_f[i] : 0;
    }
}

// One workgroup per 32 rows = one word of u; 8 threads per row.  nu_part[block] = popcount of the word.
__global__ __launch_bounds__(256) void asso_column_kernel(const uint32_t* __restrict__ X, const uint32_t* __restrict__ PD,
                                                          const uint32_t* __restrict__ b, int ldx, int m,
                                                          const uint32_t* __restrict__ tp_old, const uint32_t* __restrict__ fp_old,
                                                          double w_fp, double w_fn, uint32_t* __restrict__ u, int32_t* __restrict__ nu_part) {
    __shared__ uint32_t flag[32];
    const int t = threadIdx.x, lr = t >> 3, sub = t & 7;
    const int r = blockIdx.x * 32 + lr;
    uint32_t a = 0, ac = 0;
    for (int w = sub; w < (r < m ? ldx : 0); w += 8) {
        const uint32_t np = ~PD[(int64_t)r * ldx + w], bw = b[w];
        a += __popc(X[(int64_t)r * ldx + w] & np & bw);
        ac += __popc(np & bw);
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        a += __shfl_xor(a, o);
        ac += __shfl_xor(ac, o);
    }
    if (sub == 0) {
        bool take = false;
        if (r < m) {
            const uint32_t tpo = tp_old[r], fpo = fp_old[r];
            take = row_score(w_fp, w_fn, tpo + a, fpo + (ac - a)) > row_score(w_fp, w_fn, tpo, fpo);
        }
        flag[lr] = take ? 1u : 0u;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t word = 0;
#pragma unroll
        for (int q = 0; q < 32; ++q) word |= flag[q] << q;
        u[blockIdx.x] = word;
        nu_part[blockIdx.x] = __popc(word);
    }
}

// PD_r |= v for every row r whose bit of u is set; one wave per row, 4 rows per block
__global__ __launch_bounds__(256) void asso_apply_kernel(uint32_t* __restrict__ PD, int ldx, int m, const uint32_t* __restrict__ u,
                                                         const uint32_t* __restrict__ v) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= m || !(u[r >> 5] >> (r & 31) & 1u)) return;
    for (int w = lane; w < ldx; w += 64) PD[(int64_t)r * ldx + w] |= v[w];
}

}  // namespace

extern "C" int bmf_asso_basis(const uint32_t* Xt, int32_t n, int64_t ldw, double tau, uint32_t* B, int64_t ldb, int32_t* count,
                              void* stream) {
    BMF_REQUIRE(Xt && B && count, "bmf_asso_basis: null pointer");
    BMF_REQUIRE(n >= 1 && ldw >= 16 && ldw % 16 == 0, "bmf_asso_basis: need n >= 1 and ldw a positive multiple of 16");
    BMF_REQUIRE(ldb % 16 == 0 && ldb * 32 >= n, "bmf_asso_basis: ldb must be a multiple of 16 with ldb * 32 >= n");
    BMF_REQUIRE(ldw * 32 < ((int64_t)1 << 31), "bmf_asso_basis: too many rows for 32-bit counts");
    BMF_REQUIRE(tau == tau, "bmf_asso_basis: tau is not a number");
    BMF_REQUIRE(bmf_aligned16(Xt), "bmf_asso_basis: Xt must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const unsigned tiles = (unsigned)((n + TILE - 1) / TILE);
    BMF_LAUNCH(asso_basis_kernel, dim3(tiles, tiles), dim3(256), 0, s, Xt, n, (int)ldw, tau, B, (int)ldb);
    bits_rowcount_launch(B, n, (int)ldb, count, s);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int64_t bmf_asso_score_work(int32_t m, int32_t ncand) {
    if (m < 1 || ncand < 1) return BMF_ERR_BAD_ARG;
    return (int64_t)((m + TILE - 1) / TILE) * ncand * 16;   // bytes: one (T, F) int64 pair per (row tile, candidate)
}

extern "C" int bmf_asso_score(const uint32_t* X, const uint32_t* PD, const uint32_t* B, int64_t ldx, int32_t m, int32_t n_rows_b,
                              const int32_t* cand, int32_t ncand, const uint32_t* tp_old, const uint32_t* fp_old, double w_fp,
                              double w_fn, void* work, void* stream) {
    BMF_REQUIRE(X && PD && B && cand && tp_old && fp_old && work, "bmf_asso_score: null pointer");
    BMF_REQUIRE(m >= 1 && ncand >= 1 && n_rows_b >= 1, "bmf_asso_score: need m, ncand, n_rows_b >= 1");
    BMF_REQUIRE(ldx >= 16 && ldx % 16 == 0, "bmf_asso_score: ldx must be a positive multiple of 16");
    BMF_REQUIRE(ldx * 32 * 2 * TILE < ((int64_t)1 << 32), "bmf_asso_score: too many columns for the 32-bit tile sums");
    BMF_REQUIRE((m + TILE - 1) / TILE <= 65535, "bmf_asso_score: more than 4194240 rows");
    BMF_REQUIRE(w_fp == w_fp && w_fn == w_fn, "bmf_asso_score: a weight is not a number");
    BMF_REQUIRE(bmf_aligned16(X) && bmf_aligned16(PD) && bmf_aligned16(B), "bmf_asso_score: X, PD and B must be 16-byte aligned");
    BMF_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0, "bmf_asso_score: work must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(asso_score_kernel, dim3((unsigned)((ncand + TILE - 1) / TILE), (unsigned)((m + TILE - 1) / TILE)), dim3(256), 0, s, X, PD, B,
               (int)ldx, m, n_rows_b, cand, ncand, tp_old, fp_old, w_fp, w_fn, static_cast<int64_t*>(work));
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_asso_pick(const void* work, int32_t m, const int32_t* cand, int32_t ncand, double best_score, double w_fp, double w_fn,
                             int64_t* T, int64_t* F, double* score, int64_t* rec, void* stream) {
    BMF_REQUIRE(work && cand && T && F && score && rec, "bmf_asso_pick: null pointer");
    BMF_REQUIRE(m >= 1 && ncand >= 1, "bmf_asso_pick: need m, ncand >= 1");
    BMF_REQUIRE(best_score == best_score && w_fp == w_fp && w_fn == w_fn, "bmf_asso_pick: best_score or a weight is not a number");
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(asso_reduce_kernel, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, s, static_cast<const int64_t*>(work), (m + TILE - 1) / TILE,
               ncand, w_fp, w_fn, T, F, score);
    BMF_LAUNCH(asso_pick_kernel, dim3(1), dim3(256), 0, s, T, F, score, ncand, cand, best_score, rec);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_asso_column(const uint32_t* X, const uint32_t* PD, const uint32_t* b, int64_t ldx, int32_t m, const uint32_t* tp_old,
                               const uint32_t* fp_old, double w_fp, double w_fn, uint32_t* u, int32_t* work, int64_t* nu, void* stream) {
    BMF_REQUIRE(X && PD && b && tp_old && fp_old && u && work && nu, "bmf_asso_column: null pointer");
    BMF_REQUIRE(m >= 1 && ldx >= 1, "bmf_asso_column: need m, ldx >= 1");
    BMF_REQUIRE(w_fp == w_fp && w_fn == w_fn, "bmf_asso_column: a weight is not a number");
    hipStream_t s = (hipStream_t)stream;
    const int words = (m + 31) / 32;   // u: ceil(m / 32) words are written; work: as many int32
    BMF_LAUNCH(asso_column_kernel, dim3((unsigned)words), dim3(256), 0, s, X, PD, b, (int)ldx, m, tp_old, fp_old, w_fp, w_fn, u, work);
    bits_sum_launch(work, words, nu, nullptr, s);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_asso_apply(uint32_t* PD, int64_t ldx, int32_t m, const uint32_t* u, const uint32_t* v, void* stream) {
    BMF_REQUIRE(PD && u && v, "bmf_asso_apply: null pointer");
    BMF_REQUIRE(m >= 1 && ldx >= 1, "bmf_asso_apply: need m, ldx >= 1");
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(asso_apply_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, PD, (int)ldx, m, u, v);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
