// The bit-set kernels that no single Boolean model owns, and the entry points made of them alone.
//   bits_rowcount_kernel    count[j] = |R_j| of every bit row
//   bits_sum_kernel         the sum of n int32 counts as one int64, and how many of them are positive when that is asked for
//   bits_confusion_kernel   TP = |pd & gt|, |pd| of two bit matrices, row by row
// Integer adds in a fixed order, no atomics: the same input gives the same output whatever the grid.
#include "bits_common.h"

namespace {

// One wave per bit row, 4 rows per block.
__global__ __launch_bounds__(256) void bits_rowcount_kernel(const uint32_t* __restrict__ R, int rows, int ld, int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= rows) return;
    const uint32_t* r = R + (int64_t)j * ld;
    uint32_t c = 0;
    for (int w = lane; w < ld; w += 64) c += __popc(r[w]);
    c = wave_sum(c);
    if (lane == 0) count[j] = (int32_t)c;
}

// One block: *sum = the n counts added in a fixed order; POS: *n_pos = the number of positive counts.
template <bool POS>
__global__ __launch_bounds__(256) void bits_sum_kernel(const int32_t* __restrict__ x, int n, int64_t* __restrict__ sum, int64_t* __restrict__ n_pos) {
    __shared__ int64_t red[256];
    __shared__ int32_t pos[POS ? 256 : 1];
    const int t = threadIdx.x;
    int64_t s = 0;
    int32_t p = 0;
    for (int i = t; i < n; i += 256) {
        s += x[i];
        if (POS) p += x[i] > 0;
    }
    red[t] = s;
    if (POS) pos[t] = p;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            red[t] += red[t + o];
            if (POS) pos[t] += pos[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        sum[0] = red[0];
        if (POS) n_pos[0] = pos[0];
    }
}

// per-row |P & G| and |P| of two bit matrices (one wave per row, 4 rows per block)
__global__ __launch_bounds__(256) void bits_confusion_kernel(const uint32_t* __restrict__ P, const uint32_t* __restrict__ G, int rows, int W,
                                                             int32_t* __restrict__ tp, int32_t* __restrict__ np_) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    uint32_t a = 0, b = 0;
    for (int w = lane; w < W; w += 64) {
        const uint32_t p = P[(int64_t)r * W + w];
        a += __popc(p & G[(int64_t)r * W + w]);
        b += __popc(p);
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
        tp[r] = (int32_t)a;
        np_[r] = (int32_t)b;
    }
}

}  // namespace

void bits_rowcount_launch(const uint32_t* R, int rows, int ld, int32_t* count, hipStream_t s) {
    BMF_LAUNCH(bits_rowcount_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, R, rows, ld, count);
}

void bits_sum_launch(const int32_t* x, int n, int64_t* sum, int64_t* n_pos, hipStream_t s) {
    if (n_pos)
        BMF_LAUNCH(bits_sum_kernel<true>, dim3(1), dim3(256), 0, s, x, n, sum, n_pos);
    else
        BMF_LAUNCH(bits_sum_kernel<false>, dim3(1), dim3(256), 0, s, x, n, sum, n_pos);
}

extern "C" int bmf_bits_confusion(const uint32_t* Pbits, const uint32_t* Gbits, int32_t rows, int64_t ldw, int32_t* work, int64_t* counts,
                                  void* stream) {
    BMF_REQUIRE(Pbits && Gbits && work && counts, "bmf_bits_confusion: null pointer");
    BMF_REQUIRE(rows >= 1 && ldw >= 1, "bmf_bits_confusion: need rows, ldw >= 1");
    hipStream_t s = (hipStream_t)stream;
    BMF_LAUNCH(bits_confusion_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, Pbits, Gbits, rows, (int)ldw, work, work + rows);
    bits_sum_launch(work, rows, counts, nullptr, s);
    bits_sum_launch(work + rows, rows, counts + 1, nullptr, s);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}

extern "C" int bmf_mebf_scores(const uint32_t* R, int32_t N, int64_t ld, int32_t* score, int64_t* out, void* stream) {
    BMF_REQUIRE(R && score && out, "bmf_mebf_scores: null pointer");
    BMF_REQUIRE(N >= 1 && ld >= 1 && ld <= (1 << 26), "bmf_mebf_scores: need N >= 1 and 1 <= ld <= 2^26");
    hipStream_t s = (hipStream_t)stream;
    bits_rowcount_launch(R, N, (int)ld, score, s);
    bits_sum_launch(score, N, out, out + 1, s);
    BMF_LAUNCH_CHECK();
    return BMF_OK;
}
