// dev_scan64.hpp -- dev_scan.hpp's three-kernel exclusive scan with 64-bit sums: u32 counts in, u64
// offsets out (the complete-hit-list query's offsets: a total past 2^32 records is legitimate).  The
// block partials live in the CALLER's scratch, scan64_scratch_bytes(n), so calls may be in flight on
// several streams.  Internal linkage, like dev_scan.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace ceres {
namespace devscan64 {
namespace {

typedef unsigned long long u64;
constexpr int kScanBlock = 1024;           // elements per block (256 threads x 4)

__device__ u64 block_exclusive_scan_256(u64 v, u64* sh, u64& total) {
    // sh: 4 entries
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 x = v;
    for (int off = 1; off < 64; off <<= 1) {
        const u64 y = __shfl_up(x, off, 64);
        if (lane >= uint32_t(off)) x += y;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    u64 wbase = 0;
    for (uint32_t w = 0; w < wave; ++w) wbase += sh[w];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return wbase + x - v;
}

__global__ void __launch_bounds__(256) ceres_scan64_reduce(const uint32_t* __restrict__ in, uint32_t n, u64* __restrict__ partial) {
    __shared__ u64 sh[4];
    const uint32_t base = blockIdx.x * uint32_t(kScanBlock) + threadIdx.x * 4u;
    u64 v = 0;
    for (uint32_t k = 0; k < 4; ++k) if (base + k < n) v += in[base + k];
    u64 total;
    (void)block_exclusive_scan_256(v, sh, total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// single workgroup: exclusive scan of the block partials in place, partial[nb] = the grand total
__global__ void __launch_bounds__(256) ceres_scan64_partials(u64* partial, uint32_t nb) {
    __shared__ u64 sh[4];
    u64 carry = 0;
    for (uint32_t base = 0; base < nb; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const u64 v = i < nb ? partial[i] : 0ull;
        u64 total;
        const u64 ex = block_exclusive_scan_256(v, sh, total);
        if (i < nb) partial[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) partial[nb] = carry;
}

__global__ void __launch_bounds__(256) ceres_scan64_down(const uint32_t* __restrict__ in, uint32_t n, const u64* __restrict__ partial,
                                                         u64* __restrict__ out) {
    __shared__ u64 sh[4];
    const uint32_t base = blockIdx.x * uint32_t(kScanBlock) + threadIdx.x * 4u;
    uint32_t v[4];
    u64 sum = 0;
    for (uint32_t k = 0; k < 4; ++k) { v[k] = base + k < n ? in[base + k] : 0u; sum += v[k]; }
    u64 total;
    u64 x = partial[blockIdx.x] + block_exclusive_scan_256(sum, sh, total);
    for (uint32_t k = 0; k < 4; ++k) { if (base + k < n) out[base + k] = x; x += v[k]; }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = partial[gridDim.x];
}

// out[0..n) = exclusive prefix sums of in[0..n), out[n] = total.  partial: scan64_scratch_bytes(n).
inline uint32_t scan_blocks(size_t n) { return uint32_t((n + kScanBlock - 1) / kScanBlock); }
inline size_t scan64_scratch_bytes(size_t n) { return (size_t(scan_blocks(n)) + 1) * sizeof(u64); }
inline hipError_t exclusive_scan64(const uint32_t* in, uint32_t n, u64* out, u64* partial, hipStream_t stream) {
    const uint32_t nb = scan_blocks(n);
    if (nb == 0) return hipMemsetAsync(out, 0, sizeof(u64), stream);
    hipLaunchKernelGGL(ceres_scan64_reduce, dim3(nb), dim3(256), 0, stream, in, n, partial);
    hipLaunchKernelGGL(ceres_scan64_partials, dim3(1), dim3(256), 0, stream, partial, nb);
    hipLaunchKernelGGL(ceres_scan64_down, dim3(nb), dim3(256), 0, stream, in, n, partial, out);
    return hipGetLastError();
}

}  // namespace
}  // namespace devscan64
}  // namespace ceres
