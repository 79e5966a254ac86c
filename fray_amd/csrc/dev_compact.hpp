// Lists of active work items and their stable compaction, shared by the entries that trace lists of pixels through the frame's own path-tracing
// kernels: adaptive frames (adaptive_variant.hip) and sample maps (samplemap_variant.hip).  Each including object gets its own copy of the kernels.
#pragma once
#include "kernels.hpp"

namespace {

// The first list: work item i of the call's buckets, flagged when its pixel lies inside the frame (ragged edge buckets)
static __global__ __launch_bounds__(256) void k_list_init(DFrame F, int nItems, int* __restrict__ list, unsigned char* __restrict__ flag)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nItems; i += gridDim.x * blockDim.x) {
        int x, y;
        list[i] = i;
        flag[i] = item_pixel(F, i, x, y) ? 1 : 0;
    }
}

// ---- stable compaction of the list by its flags: tiles of 2048 entries (8 consecutive per thread), their counts, one exclusive scan of the
// counts, then every tile writes its flagged entries in order at its offset.  *count receives the new length.
constexpr int kPerThread = 8, kTile = 256 * kPerThread;

static __global__ __launch_bounds__(256) void k_compact_count(const unsigned char* __restrict__ flag, int n, int* __restrict__ tileCount)
{
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const int base = blockIdx.x * kTile + threadIdx.x * kPerThread;
    int c = 0;
    for (int k = 0; k < kPerThread; k++) if (base + k < n && flag[base + k]) c++;
    if (c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0) tileCount[blockIdx.x] = total;
}

// Inclusive scan of one value per thread over a block of 1024 (Hillis-Steele in LDS)
FD int block_scan_1024(int v, int* lds)
{
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int t = threadIdx.x >= (unsigned)d ? lds[threadIdx.x - d] : 0;
        __syncthreads();
        lds[threadIdx.x] += t;
        __syncthreads();
    }
    const int r = lds[threadIdx.x];
    __syncthreads();
    return r;
}

static __global__ __launch_bounds__(1024) void k_compact_scan(const int* __restrict__ tileCount, int nTiles, int* __restrict__ tileOffset, int* __restrict__ count)
{
    __shared__ int lds[1024];
    int carry = 0;
    for (int t0 = 0; t0 < nTiles; t0 += 1024) {
        const int t = t0 + (int)threadIdx.x;
        const int v = t < nTiles ? tileCount[t] : 0;
        const int incl = block_scan_1024(v, lds);
        if (t < nTiles) tileOffset[t] = carry + incl - v;
        carry += lds[1023];                                     // the chunk's total (block_scan_1024 leaves the scan in lds)
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}

static __global__ __launch_bounds__(256) void k_compact_write(const int* __restrict__ list, const unsigned char* __restrict__ flag, int n,
                                                              const int* __restrict__ tileOffset, int* __restrict__ out)
{
    __shared__ int lds[256];
    const int base = blockIdx.x * kTile + threadIdx.x * kPerThread;
    int c = 0;
    for (int k = 0; k < kPerThread; k++) if (base + k < n && flag[base + k]) c++;
    lds[threadIdx.x] = c;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int t = threadIdx.x >= (unsigned)d ? lds[threadIdx.x - d] : 0;
        __syncthreads();
        lds[threadIdx.x] += t;
        __syncthreads();
    }
    int o = tileOffset[blockIdx.x] + lds[threadIdx.x] - c;
    for (int k = 0; k < kPerThread; k++)
        if (base + k < n && flag[base + k]) out[o++] = list[base + k];
}

}  // namespace
