// What the bit-set kernels of the Boolean models share (grecond / grecondplus / asso / mebf / panda .hip): 16-byte word helpers, the
// argument checks of their entry points, and the two launches of bits_common.hip.  Integers and bits only: several includers are
// built with -ffp-contract=off, and nothing here may depend on that.
#pragma once
#include "common.h"

__device__ inline int popc4(uint4 v) { return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }
__device__ inline uint4 and4(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }
__device__ inline uint4 andn4(uint4 a, uint4 b) { return make_uint4(a.x & ~b.x, a.y & ~b.y, a.z & ~b.z, a.w & ~b.w); }

// host: a leading dimension that 16-byte loads can walk; pointer alignment (a null pointer passes)
static inline bool ld_ok(int64_t ld) { return ld >= 4 && ld % 4 == 0 && ld <= (1 << 26); }
static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// Enqueue only: the caller checks the launches of its entry point once, behind the last of them.
// count[j] = |R_j| for the `rows` bit rows of ld words (one wave per row, 4 rows per block)
void bits_rowcount_launch(const uint32_t* R, int rows, int ld, int32_t* count, hipStream_t s);
// One block: *sum = the n counts added in a fixed order; n_pos (may be null) = how many of them are positive
void bits_sum_launch(const int32_t* x, int n, int64_t* sum, int64_t* n_pos, hipStream_t s);
