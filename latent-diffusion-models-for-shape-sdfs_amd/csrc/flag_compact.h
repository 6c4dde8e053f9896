// The block scan of mc.hip, band.hip and sdf_trace.hip, and the flag compaction of the last two:
// `nseg` segments of `n` byte flags each -> per segment the indices of its set flags in
// ascending order and their number.  Block sums + chunk scan + scatter, no atomic append and no
// workgroup waiting on another: the lists are a pure function of the flags, whatever the
// scheduling.  Everything here runs 256 threads per workgroup.
#pragma once
#include "ldm_internal.h"

namespace ldm {

// block-wide exclusive scan of one int per thread (256 threads); the block total through *total
__device__ __forceinline__ int block_excl_scan(int v, int* lds /*[4]*/, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wv] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wv) base += lds[w];
        tot += lds[w];
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

namespace {

// flags per thread of the compaction passes (one 16-byte vector), a chunk = 256 threads
constexpr int kFlagsPer = 16;
constexpr int kFlagChunk = 256 * kFlagsPer;
inline int64_t flag_chunks(int64_t n) { return (n + kFlagChunk - 1) / kFlagChunk; }

// This thread's 16 flags of chunk blockIdx.x of segment blockIdx.y as a bit mask (zeros past n);
// *p0 = the index of bit 0 in the segment, 64-bit: n can be near 2^31 and the last chunk's
// threads start past it.  One 16-byte load where all 16 flags exist and their address is
// 16-byte aligned (a segment starts at seg * n, aligned only when n % 16 == 0), else byte loads.
__device__ __forceinline__ unsigned load_flags(const uint8_t* __restrict__ flags, int n,
                                               int64_t* p0) {
    *p0 = (int64_t)blockIdx.x * kFlagChunk + threadIdx.x * kFlagsPer;
    const uint8_t* f = flags + (int64_t)blockIdx.y * n + *p0;
    unsigned m = 0;
    if (*p0 + kFlagsPer <= n && LDM_ALIGNED(f, 16)) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(f);
#pragma unroll
        for (int q = 0; q < kFlagsPer; ++q)
            m |= (((a[q >> 2] >> (8 * (q & 3))) & 0xffu) ? 1u : 0u) << q;
    } else {
#pragma unroll
        for (int q = 0; q < kFlagsPer; ++q) m |= ((*p0 + q < n && f[q]) ? 1u : 0u) << q;
    }
    return m;
}

// grid (nchunk, nseg): bsum[seg][chunk] = the chunk's set flags
__global__ __launch_bounds__(256) void flag_block_sums_kernel(const uint8_t* __restrict__ flags,
                                                              int n, int* __restrict__ bsum) {
    __shared__ int lds[4];
    int64_t p0;
    int tot;
    block_excl_scan(__popc(load_flags(flags, n, &p0)), lds, &tot);
    if (threadIdx.x == 0) bsum[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// grid (nseg): one workgroup scans one segment's chunk sums (thread t owns the chunks
// [t per, (t + 1) per), summed serially, one block scan of the 256 thread sums, a second serial
// pass writes the exclusive offsets); counts[seg] = the segment's set flags
__global__ __launch_bounds__(256) void flag_chunk_scan_kernel(const int* __restrict__ bsum,
                                                              int nchunk, int* __restrict__ boff,
                                                              int32_t* __restrict__ counts) {
    __shared__ int lds[4];
    const int* in = bsum + (int64_t)blockIdx.x * nchunk;
    int* out = boff + (int64_t)blockIdx.x * nchunk;
    const int per = (nchunk + 255) / 256;
    const int b0 = min((int)threadIdx.x * per, nchunk), b1 = min(b0 + per, nchunk);
    int sum = 0;
    for (int c = b0; c < b1; ++c) sum += in[c];
    int tot;
    int c0 = block_excl_scan(sum, lds, &tot);
    for (int c = b0; c < b1; ++c) {
        out[c] = c0;
        c0 += in[c];
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = tot;
}

// grid (nchunk, nseg): list[seg n + k] = the segment's k-th set flag
__global__ __launch_bounds__(256) void flag_scatter_kernel(const uint8_t* __restrict__ flags,
                                                           int n, const int* __restrict__ boff,
                                                           int32_t* __restrict__ list) {
    __shared__ int lds[4];
    int64_t p0;
    unsigned m = load_flags(flags, n, &p0);
    int tot;
    int off = boff[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] +
              block_excl_scan(__popc(m), lds, &tot);
    int32_t* dst = list + (int64_t)blockIdx.y * n;
    while (m) {
        const int q = __builtin_ctz(m);
        m &= m - 1u;
        dst[off++] = (int32_t)(p0 + q);     // a set flag: p0 + q < n < 2^31; off < the count <= n
    }
}

struct FlagCompactWs {
    int* bsum;      // [nseg][nchunk]
    int* boff;      // [nseg][nchunk]
    size_t bytes;
};

// the two arrays laid out from `base` (256-byte aligned, may be NULL for the byte count alone)
inline FlagCompactWs flag_compact_ws(int nseg, int64_t n, void* base) {
    const size_t each = up256((size_t)nseg * (size_t)flag_chunks(n) * sizeof(int));
    char* b = reinterpret_cast<char*>(base);
    return {reinterpret_cast<int*>(b), reinterpret_cast<int*>(b + each), 2 * each};
}

// The three launches.  flags [nseg][n], list [nseg][n], counts [nseg]; the caller has checked
// nseg n < 2^31 and that the chunks and the segments fit their grid axes.
inline void flag_compact(const uint8_t* flags, int nseg, int n, const FlagCompactWs& w,
                         int32_t* list, int32_t* counts, hipStream_t st) {
    const int nchunk = (int)flag_chunks(n);
    hipLaunchKernelGGL(flag_block_sums_kernel, dim3(nchunk, nseg), dim3(256), 0, st, flags, n,
                       w.bsum);
    hipLaunchKernelGGL(flag_chunk_scan_kernel, dim3(nseg), dim3(256), 0, st, w.bsum, nchunk,
                       w.boff, counts);
    hipLaunchKernelGGL(flag_scatter_kernel, dim3(nchunk, nseg), dim3(256), 0, st, flags, n, w.boff,
                       list);
}

}  // namespace
}  // namespace ldm
