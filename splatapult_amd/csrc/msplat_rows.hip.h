// msplat_rows.hip.h -- the row reduction msplat_measure_cloud and msplat_histogram_values end with: every lane accumulates a Row, the
// lanes' rows become one row per workgroup (row_reduce_store), the workgroups' rows one row (rows_finish_kernel).  No atomics, and a
// merge order fixed by the grid alone -- the lane's own loop, the wave butterfly from 32 down to 1, the waves in wave order, the
// finish rows in lane stride -- so a call repeated on a context returns the same bytes.  A Row is trivially copyable, a multiple of
// 4 bytes, and has clear() (the empty row) and merge(const Row&): a new field is written in those two and nowhere else.
// (Included by msplat_kernels.hip.h before msplat_select.hip.h; host side: reduce_rows, msplat_edit.hip.inc.  NOT of this shape:
// cloud_moments_kernel / _finish, whose finish is another tree and whose bits decide the Morton storage order; the 7-float boxes.)
#pragma once

#include <type_traits>

#include "msplat_common.hip.h"

namespace msplat {

// every lane's row -> one row per workgroup: butterflies inside the wave, then the waves' rows in wave order through LDS.  The
// partner lane's row moves as 32-bit words (a double as its two halves: the bits __shfl_xor(double) carries)
template <class Row>
__device__ __forceinline__ void row_reduce_store(Row& r, Row* __restrict__ out)
{
    static_assert(std::is_trivially_copyable<Row>::value && sizeof(Row) % 4 == 0, "a row is shuffled as 32-bit words");
    __shared__ Row s_w[kThreads / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        uint32_t w[sizeof(Row) / 4];
        __builtin_memcpy(w, &r, sizeof(Row));
#pragma unroll
        for (uint32_t& v : w) v = __shfl_xor(v, d, 64);
        Row o;
        __builtin_memcpy(&o, w, sizeof(Row));
        r.merge(o);
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        Row t = s_w[0];
        for (int w = 1; w < kThreads / 64; ++w) t.merge(s_w[w]);
        *out = t;
    }
}

// one workgroup: the rows of a partial pass (one per workgroup of it), in row order per lane, into *out
template <class Row>
__global__ __launch_bounds__(kThreads) void rows_finish_kernel(const Row* __restrict__ part, uint32_t rows, Row* __restrict__ out)
{
    Row r;
    r.clear();
    for (uint32_t k = threadIdx.x; k < rows; k += kThreads) r.merge(part[k]);
    row_reduce_store(r, out);
}

}  // namespace msplat
