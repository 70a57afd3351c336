// Max-sum message passing for Boolean factorisation and completion (Ravanbakhsh, Poczos, Greiner, ICML 2016, Algorithm 1), fp64 end
// to end.  The reference's wrapper (PyBMF/models/MessagePassing.py) imports the algorithm from a module that is not in its tree;
// DESIGN 9.4 defines what is computed here.
//
//   state     hats Phi^, Psi^: k planes of m x ldn doubles each (ldn = n rounded up to 64; a lane owns a column, so a wave reads a
//             plane in contiguous 512-byte lines), zero outside the observed cells; marginals Xi [m][k], Ups [k][ldn]
//   one step  every observed cell (i, j), from the OLD Xi, Ups and its own old hats:
//               Phi_f = Xi[i][f] - Phi^_f,  Psi_f = Ups[f][j] - Psi^_f,  G_f = min(Phi_f + Psi_f, Phi_f, Psi_f)
//               T = sum_f max(G_f, 0) in the order f = 0 .. k - 1,  M_f = max over f' != f of G_f' (-inf at k = 1)
//               G^_f = min(max(-M_f, 0), (T - max(G_f, 0)) + co),   co = co1 where X = 1, co0 where X = 0
//               Phi^'_f = max(G^_f + Psi_f, 0) - max(Psi_f, 0),     Psi^'_f = max(G^_f + Phi_f, 0) - max(Phi_f, 0)
//               Phi^_f <- (1 - lr) Phi^_f + lr Phi^'_f   (two products and a sum: this file is built with -ffp-contract=off)
//             then Xi = cx + row sums of Phi^, Ups = cy + column sums of Psi^, d = the largest change of a marginal
//
// min / max are the selections a < b ? a : b and a > b ? a : b (the second operand on equality, so the sign of a zero is defined and
// max(x, 0) is never -0).  The cell pass leaves one partial of every row sum per 64-column tile (the lanes of a wave added by the
// xor butterfly) and one partial of every column sum per 32-row segment (added down the rows in the lane that owns the column); the
// finish launch adds the partials in ascending tile order and the prior last.  No floating-point atomics: the same call gives the
// same bits.
#include "common.h"

namespace {

constexpr int RW = 32;   // rows of a wave's segment
constexpr int RB = 8;    // rows of a batch of the two-sweep form (their T, m1, m2 stay in registers between the sweeps)
constexpr int WV = 4;    // waves of a workgroup: four consecutive row segments of one column tile

__device__ __forceinline__ double mn(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double mx(double a, double b) { return a > b ? a : b; }

__device__ __forceinline__ double mp_gamma(double ph, double ps) { return mn(mn(ph + ps, ph), ps); }

// the two largest values of G seen so far, equal values counted twice
__device__ __forceinline__ void mp_top2(double g, double& m1, double& m2) {
    const double lo = g > m2 ? g : m2;   // (selections, not branches on references: those went through scratch memory)
    m2 = g > m1 ? m1 : lo;
    m1 = g > m1 ? g : m1;
}

// The new hats of one (cell, f) from its old hats (a, b), Phi_f, Psi_f, G_f and the cell's T, m1, m2.
__device__ __forceinline__ void mp_update(double ph, double ps, double g, double T, double m1, double m2, double co, double oml, double lr,
                                          double& a, double& b) {
    const double M = g == m1 ? m2 : m1;
    const double gh = mn(mx(-M, 0.0), (T - mx(g, 0.0)) + co);
    const double pn = mx(gh + ps, 0.0) - mx(ps, 0.0);
    const double qn = mx(gh + ph, 0.0) - mx(ph, 0.0);
    a = oml * a + lr * pn;
    b = oml * b + lr * qn;
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct mp_tile {
    int lane, tc, rs, rows;   // lane; column tile; row segment; rows of the segment inside the matrix (0: nothing to do)
    int64_t i0, j;            // first row; this lane's column
};

__device__ __forceinline__ mp_tile mp_tile_of(int m, int nrs) {
    mp_tile t;
    t.lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    t.tc = blockIdx.x;
    t.rs = blockIdx.y * WV + wave;
    t.i0 = (int64_t)t.rs * RW;
    t.rows = t.rs < nrs ? (int)min((int64_t)RW, (int64_t)m - t.i0) : 0;
    t.j = (int64_t)blockIdx.x * 64 + t.lane;
    return t;
}

// is cell (i, j) observed / a one: bit j of row i of a bit matrix with ldx words per row
__device__ __forceinline__ bool mp_bit(const uint32_t* __restrict__ bits, int64_t ldx, int64_t i, int64_t j) {
    return (bits[i * ldx + (j >> 5)] >> (j & 31)) & 1u;
}

// ---- start: the counter-based fill ------------------------------------------------------------------------------------------------
// hat `which` (0: Phi^, 1: Psi^) of cell (i, j), factor f := init_scale (2 u - 1), u = the top 53 bits of
// splitmix64(splitmix64(seed) + ((which m + i) n + j) k + f) as a fraction; 0 outside the pattern and in the padding columns.
template <bool MASK>
__global__ __launch_bounds__(256) void mp_start_kernel(const uint32_t* __restrict__ Wbits, int64_t ldx, int m, int n, int k, int64_t ldn,
                                                       int nrs, uint64_t base, double init_scale, double* __restrict__ Phi,
                                                       double* __restrict__ Psi) {
    const mp_tile t = mp_tile_of(m, nrs);
    const int64_t plane = (int64_t)m * ldn;
    for (int r = 0; r < t.rows; ++r) {
        const int64_t i = t.i0 + r;
        const bool obs = t.j < n && (!MASK || mp_bit(Wbits, ldx, i, t.j));
        const uint64_t c0 = (((uint64_t)i * (uint64_t)n + (uint64_t)t.j) * (uint64_t)k);
        const uint64_t c1 = ((((uint64_t)m + (uint64_t)i) * (uint64_t)n + (uint64_t)t.j) * (uint64_t)k);
        for (int f = 0; f < k; ++f) {
            const double u0 = (double)(splitmix64(base + c0 + f) >> 11) * 0x1.0p-53;
            const double u1 = (double)(splitmix64(base + c1 + f) >> 11) * 0x1.0p-53;
            const int64_t at = f * plane + i * ldn + t.j;
            Phi[at] = obs ? init_scale * (2.0 * u0 - 1.0) : 0.0;
            Psi[at] = obs ? init_scale * (2.0 * u1 - 1.0) : 0.0;
        }
    }
}

// ---- the partial sums of hats as they stand (after the start; bmf_mp_reduce) ----------------------------------------------------------
__global__ __launch_bounds__(256) void mp_sum_kernel(const double* __restrict__ Phi, const double* __restrict__ Psi, int m, int k,
                                                     int64_t ldn, int nrs, double* __restrict__ xi_part, double* __restrict__ ups_part) {
    const mp_tile t = mp_tile_of(m, nrs);
    if (t.rows <= 0) return;
    const int64_t plane = (int64_t)m * ldn;
    for (int f = 0; f < k; ++f) {
        double acc = 0.0;
        for (int r = 0; r < t.rows; ++r) {
            const int64_t i = t.i0 + r, at = f * plane + i * ldn + t.j;
            const double s = wave_sum(Phi[at]);
            acc += Psi[at];
            if (t.lane == 0) xi_part[((int64_t)t.tc * m + i) * k + f] = s;
        }
        ups_part[((int64_t)t.rs * k + f) * ldn + t.j] = acc;
    }
}

// ---- the cell pass, k <= KT: a cell's 2 k hats stay in registers, every plane is read once and written once ---------------------------
template <int KT, bool MASK>
__global__ __launch_bounds__(256) void mp_cell_kernel(const uint32_t* __restrict__ Xbits, const uint32_t* __restrict__ Wbits, int64_t ldx,
                                                      int m, int n, int k, int64_t ldn, int nrs, double co1, double co0, double oml,
                                                      double lr, const double* __restrict__ Xi, const double* __restrict__ Ups,
                                                      double* __restrict__ Phi, double* __restrict__ Psi, double* __restrict__ xi_part,
                                                      double* __restrict__ ups_part) {
    const mp_tile t = mp_tile_of(m, nrs);
    if (t.rows <= 0) return;
    const int64_t plane = (int64_t)m * ldn;
    double up[KT], acc[KT];
#pragma unroll
    for (int f = 0; f < KT; ++f) {
        up[f] = f < k ? Ups[f * ldn + t.j] : 0.0;
        acc[f] = 0.0;
    }
    for (int r = 0; r < t.rows; ++r) {
        const int64_t i = t.i0 + r, at = i * ldn + t.j;
        const bool obs = t.j < n && (!MASK || mp_bit(Wbits, ldx, i, t.j));
        const double co = mp_bit(Xbits, ldx, i, t.j) ? co1 : co0;
        const double* __restrict__ xi = Xi + i * k;
        double a[KT], b[KT];
#pragma unroll
        for (int f = 0; f < KT; ++f)
            if (f < k) {
                a[f] = Phi[f * plane + at];
                b[f] = Psi[f * plane + at];
            }
        double T = 0.0, m1 = -INFINITY, m2 = -INFINITY;
#pragma unroll
        for (int f = 0; f < KT; ++f)
            if (f < k) {
                const double g = mp_gamma(xi[f] - a[f], up[f] - b[f]);
                T = T + mx(g, 0.0);
                mp_top2(g, m1, m2);
            }
#pragma unroll
        for (int f = 0; f < KT; ++f)
            if (f < k) {
                const double ph = xi[f] - a[f], ps = up[f] - b[f];
                double an = a[f], bn = b[f];
                mp_update(ph, ps, mp_gamma(ph, ps), T, m1, m2, co, oml, lr, an, bn);
                if (obs) {
                    Phi[f * plane + at] = an;
                    Psi[f * plane + at] = bn;
                }
                acc[f] += obs ? bn : 0.0;
                const double s = wave_sum(obs ? an : 0.0);
                if (t.lane == 0) xi_part[((int64_t)t.tc * m + i) * k + f] = s;
            }
    }
#pragma unroll
    for (int f = 0; f < KT; ++f)
        if (f < k) ups_part[((int64_t)t.rs * k + f) * ldn + t.j] = acc[f];
}

// ---- the cell pass, any k <= 64, in two sweeps over the planes: sweep 1 forms T and the two largest G of RB rows' cells, sweep 2 reads
// the planes again, factor by factor, and writes the new hats (6 x 8 k bytes per cell instead of 4 x 8 k) ------------------------------
template <bool MASK>
__global__ __launch_bounds__(256) void mp_cell2_kernel(const uint32_t* __restrict__ Xbits, const uint32_t* __restrict__ Wbits, int64_t ldx,
                                                       int m, int n, int k, int64_t ldn, int nrs, double co1, double co0, double oml,
                                                       double lr, const double* __restrict__ Xi, const double* __restrict__ Ups,
                                                       double* __restrict__ Phi, double* __restrict__ Psi, double* __restrict__ xi_part,
                                                       double* __restrict__ ups_part) {
    const mp_tile t = mp_tile_of(m, nrs);
    if (t.rows <= 0) return;
    const int64_t plane = (int64_t)m * ldn;
    for (int r0 = 0; r0 < t.rows; r0 += RB) {
        const int nr = min(RB, t.rows - r0);   // wave-uniform
        const int64_t ib = t.i0 + r0;
        double T[RB], m1[RB], m2[RB], co[RB];
        bool obs[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            T[r] = 0.0;
            m1[r] = m2[r] = -INFINITY;
            obs[r] = false;
            co[r] = co0;
            if (r < nr) {
                obs[r] = t.j < n && (!MASK || mp_bit(Wbits, ldx, ib + r, t.j));
                co[r] = mp_bit(Xbits, ldx, ib + r, t.j) ? co1 : co0;
            }
        }
        for (int f = 0; f < k; ++f) {
            const double up = Ups[f * ldn + t.j];
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (r < nr) {
                    const int64_t at = f * plane + (ib + r) * ldn + t.j;
                    const double g = mp_gamma(Xi[(ib + r) * k + f] - Phi[at], up - Psi[at]);
                    T[r] = T[r] + mx(g, 0.0);
                    mp_top2(g, m1[r], m2[r]);
                }
        }
        for (int f = 0; f < k; ++f) {
            const double up = Ups[f * ldn + t.j];
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (r < nr) {
                    const int64_t at = f * plane + (ib + r) * ldn + t.j;
                    double an = Phi[at], bn = Psi[at];
                    const double ph = Xi[(ib + r) * k + f] - an, ps = up - bn;
                    mp_update(ph, ps, mp_gamma(ph, ps), T[r], m1[r], m2[r], co[r], oml, lr, an, bn);
                    if (obs[r]) {
                        Phi[at] = an;
                        Psi[at] = bn;
                    }
                    acc += obs[r] ? bn : 0.0;
                    const double s = wave_sum(obs[r] ? an : 0.0);
                    if (t.lane == 0) xi_part[((int64_t)t.tc * m + ib + r) * k + f] = s;
                }
            // the segment's column partial: the first batch stores it, the later ones add to it (the same lane, in row order)
            double* dst = ups_part + ((int64_t)t.rs * k + f) * ldn + t.j;
            *dst = r0 == 0 ? acc : *dst + acc;
        }
    }
}

// ---- finish: the partials in ascending tile order, the prior last; the largest change of a marginal per workgroup -------------------
// Blocks [0, gx): Xi[i][f], one thread each; blocks [gx, gx + gu): Ups[f][j], j < n.
__global__ __launch_bounds__(256) void mp_finish_kernel(const double* __restrict__ xi_part, int ntc, int m, int k, double cx,
                                                        double* __restrict__ Xi, int gx, const double* __restrict__ ups_part, int nrs,
                                                        int64_t ldn, int n, double cy, double* __restrict__ Ups,
                                                        double* __restrict__ bmax) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double d = 0.0;
    if ((int)blockIdx.x < gx) {
        const int64_t e = (int64_t)blockIdx.x * 256 + t, cnt = (int64_t)m * k;
        if (e < cnt) {
            double s = 0.0;
            for (int c = 0; c < ntc; ++c) s += xi_part[c * cnt + e];
            s = s + cx;
            d = fabs(s - Xi[e]);
            Xi[e] = s;
        }
    } else {
        const int64_t e = (int64_t)(blockIdx.x - gx) * 256 + t, cnt = (int64_t)k * ldn;
        if (e < cnt && e % ldn < n) {
            double s = 0.0;
            for (int r = 0; r < nrs; ++r) s += ups_part[r * cnt + e];
            s = s + cy;
            d = fabs(s - Ups[e]);
            Ups[e] = s;
        }
    }
    red[t] = d;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] = mx(red[t], red[t + o]);
        __syncthreads();
    }
    if (t == 0) bmax[blockIdx.x] = red[0];
}

// Block 0: d = the largest of the nb workgroup maxima.  Blocks [1, 1 + gb) (when the decisions are asked for): word i of ubits = the
// bits Xi[i][f] > 0, word j of vbits = the bits Ups[f][j] > 0, bit f of a 64-bit word.
__global__ __launch_bounds__(256) void mp_final_kernel(const double* __restrict__ bmax, int nb, double* __restrict__ d,
                                                       const double* __restrict__ Xi, int m, int k, const double* __restrict__ Ups,
                                                       int64_t ldn, int n, uint64_t* __restrict__ ubits, uint64_t* __restrict__ vbits) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        double v = 0.0;
        for (int q = t; q < nb; q += 256) v = mx(v, bmax[q]);
        red[t] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) red[t] = mx(red[t], red[t + o]);
            __syncthreads();
        }
        if (t == 0) d[0] = red[0];
        return;
    }
    const int64_t e = (int64_t)(blockIdx.x - 1) * 256 + t;
    if (e < m) {
        uint64_t w = 0;
        for (int f = 0; f < k; ++f) w |= (uint64_t)(Xi[e * k + f] > 0.0) << f;
        ubits[e] = w;
    } else if (e - m < n) {
        const int64_t j = e - m;
        uint64_t w = 0;
        for (int f = 0; f < k; ++f) w |= (uint64_t)(Ups[f * ldn + j] > 0.0) << f;
        vbits[j] = w;
    }
}

struct mp_plan {
    int64_t ntc, nrs, xi_part, ups_part, gx, gu;   // tiles; sizes of the partial slabs in doubles; blocks of the finish launch
};

bool mp_plan_of(int64_t m, int64_t n, int k, mp_plan& p) {
    if (m < 1 || n < 1 || k < 1 || k > 64 || m > INT32_MAX || n > INT32_MAX - 64) return false;
    const int64_t ldn = (n + 63) / 64 * 64;
    p.ntc = ldn / 64;
    p.nrs = (m + RW - 1) / RW;
    p.xi_part = p.ntc * m * k;
    p.ups_part = p.nrs * k * ldn;
    p.gx = (m * k + 255) / 256;
    p.gu = (k * ldn + 255) / 256;
    return (p.nrs + WV - 1) / WV <= 65535 && p.gx + p.gu < INT32_MAX;
}

// the finish and final launches shared by bmf_mp_reduce and bmf_mp_step
int mp_finish(const mp_plan& p, int32_t m, int32_t n, int k, int64_t ldn, double cx, double cy, double* work, double* Xi, double* Ups,
              double* d, uint64_t* ubits, uint64_t* vbits, hipStream_t s) {
    double* xi_part = work;
    double* ups_part = xi_part + p.xi_part;
    double* bmax = ups_part + p.ups_part;
    const int nb = (int)(p.gx + p.gu);
    BMF_LAUNCH(mp_finish_kernel, dim3((unsigned)nb), dim3(256), 0, s, xi_part, (int)p.ntc, m, k, cx, Xi, (int)p.gx, ups_part, (int)p.nrs,
               ldn, n, cy, Ups, bmax);
    const int gb = ubits ? (int)(((int64_t)m + n + 255) / 256) : 0;
    BMF_LAUNCH(mp_final_kernel, dim3((unsigned)(1 + gb)), dim3(256), 0, s, bmax, nb, d, Xi, m, k, Ups, ldn, n, ubits, vbits);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

}  // namespace

extern "C" int64_t bmf_mp_work(int32_t m, int32_t n, int k) {
    mp_plan p;
    if (!mp_plan_of(m, n, k, p)) return BMF_ERR_BAD_ARG;
    return p.xi_part + p.ups_part + p.gx + p.gu;
}

#define BMF_MP_SHAPE(name_)                                                                                              \
    BMF_REQUIRE(m >= 1 && n >= 1, name_ ": m=%d, n=%d must be >= 1", (int)m, (int)n);                                    \
    BMF_REQUIRE(k >= 1 && k <= 64, name_ ": k=%d outside 1..64", k);                                                     \
    BMF_REQUIRE(ldn % 64 == 0 && ldn >= n && ldn < (int64_t)n + 64, name_ ": ldn=%lld is not n=%d rounded up to 64", (long long)ldn, (int)n); \
    mp_plan p;                                                                                                           \
    BMF_REQUIRE(mp_plan_of(m, n, k, p), name_ ": shape too large")

extern "C" int bmf_mp_start(const uint32_t* Wbits, int64_t ldx, int32_t m, int32_t n, int k, int64_t ldn, uint64_t seed, double init_scale,
                            double* Phi, double* Psi, void* stream) {
    BMF_REQUIRE(Phi && Psi, "bmf_mp_start: null pointer");
    BMF_MP_SHAPE("bmf_mp_start");
    BMF_REQUIRE(!Wbits || ldx * 32 >= ldn, "bmf_mp_start: ldx=%lld words do not cover ldn=%lld", (long long)ldx, (long long)ldn);
    uint64_t base = seed + 0x9E3779B97F4A7C15ull;   // splitmix64(seed), on the host
    base = (base ^ (base >> 30)) * 0xBF58476D1CE4E5B9ull;
    base = (base ^ (base >> 27)) * 0x94D049BB133111EBull;
    base ^= base >> 31;
    dim3 grid((unsigned)p.ntc, (unsigned)((p.nrs + WV - 1) / WV)), block(256);
    if (Wbits) BMF_LAUNCH(mp_start_kernel<true>, grid, block, 0, (hipStream_t)stream, Wbits, ldx, m, n, k, ldn, (int)p.nrs, base, init_scale, Phi, Psi);
    else BMF_LAUNCH(mp_start_kernel<false>, grid, block, 0, (hipStream_t)stream, Wbits, ldx, m, n, k, ldn, (int)p.nrs, base, init_scale, Phi, Psi);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_mp_reduce(const double* Phi, const double* Psi, int32_t m, int32_t n, int k, int64_t ldn, double cx, double cy,
                             double* work, double* Xi, double* Ups, double* d, uint64_t* ubits, uint64_t* vbits, void* stream) {
    BMF_REQUIRE(Phi && Psi && work && Xi && Ups && d, "bmf_mp_reduce: null pointer");
    BMF_REQUIRE(!ubits == !vbits, "bmf_mp_reduce: ubits and vbits come together");
    BMF_MP_SHAPE("bmf_mp_reduce");
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)p.ntc, (unsigned)((p.nrs + WV - 1) / WV)), block(256);
    BMF_LAUNCH(mp_sum_kernel, grid, block, 0, s, Phi, Psi, m, k, ldn, (int)p.nrs, work, work + p.xi_part);
    return mp_finish(p, m, n, k, ldn, cx, cy, work, Xi, Ups, d, ubits, vbits, s);
}

extern "C" int bmf_mp_step(const uint32_t* Xbits, const uint32_t* Wbits, int64_t ldx, int32_t m, int32_t n, int k, int64_t ldn, double co1,
                           double co0, double lr, double cx, double cy, double* Phi, double* Psi, double* work, double* Xi, double* Ups,
                           double* d, uint64_t* ubits, uint64_t* vbits, void* stream) {
    BMF_REQUIRE(Xbits && Phi && Psi && work && Xi && Ups && d, "bmf_mp_step: null pointer");
    BMF_REQUIRE(!ubits == !vbits, "bmf_mp_step: ubits and vbits come together");
    BMF_MP_SHAPE("bmf_mp_step");
    BMF_REQUIRE(ldx * 32 >= ldn, "bmf_mp_step: ldx=%lld words do not cover ldn=%lld", (long long)ldx, (long long)ldn);
    BMF_REQUIRE(co1 == co1 && co0 == co0 && lr == lr, "bmf_mp_step: NaN constant");
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)p.ntc, (unsigned)((p.nrs + WV - 1) / WV)), block(256);
    double* xi_part = work;
    double* ups_part = work + p.xi_part;
    const double oml = 1.0 - lr;
#define BMF_MP_CELL(kernel_)                                                                                                        \
    BMF_LAUNCH((kernel_), grid, block, 0, s, Xbits, Wbits, ldx, m, n, k, ldn, (int)p.nrs, co1, co0, oml, lr, Xi, Ups, Phi, Psi, xi_part, ups_part)
    if (k <= 8) { if (Wbits) BMF_MP_CELL((mp_cell_kernel<8, true>)); else BMF_MP_CELL((mp_cell_kernel<8, false>)); }
    else if (k <= 16) { if (Wbits) BMF_MP_CELL((mp_cell_kernel<16, true>)); else BMF_MP_CELL((mp_cell_kernel<16, false>)); }
    else { if (Wbits) BMF_MP_CELL(mp_cell2_kernel<true>); else BMF_MP_CELL(mp_cell2_kernel<false>); }
#undef BMF_MP_CELL
    return mp_finish(p, m, n, k, ldn, cx, cy, work, Xi, Ups, d, ubits, vbits, s);
}
