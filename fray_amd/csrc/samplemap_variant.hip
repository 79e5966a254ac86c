// Sample maps (frayhip_render_samples_map, include/frayhip.h) for one kernel flag word: the Makefile compiles this file eight times, -DFRAY_ST=0..5,
// 8, 9, into samplemap<ST>.o.  A resumable state (frayhip_render_samples' rows) whose pixels each take as many more samples as the caller's `add`
// plane says, traced through the frame's own exact path-tracing kernels as adaptive frames are (kernels.hpp is not touched, only instantiated here
// once more).
//
// The call works in LAYERS of at most cn samples per pixel.  The layer at offset k0 lists the pixels with add > k0 (ascending work items, so
// neighbouring list entries are neighbouring pixels of one 8x8 tile); entry i takes c_i = min(cn, add_i - k0) samples, its samples
// count_i + k0 .. count_i + k0 + c_i - 1.  A batch is a range of list entries; an exclusive scan of their c_i gives every entry a contiguous
// range of slots, so the batch is dense whatever the map looks like: no slot without a sample somebody asked for.
//   k_map_init           the first list (work items of the call's buckets with add > 0), the planes' check, sum and maximum of add
//   k_map_count / k_compact_scan / k_map_offsets   the exclusive scan of c_i over a batch's entries (tiles of 2048, as the compaction)
//   k_map_expand         slot -> entry index (a binary search in the offsets)
//   k_seed_map           k_seed_list with (pixel, sample) looked up per slot
//   k_pt_init_map<ST>    k_pt_init_list likewise
//   then the frame's own exact kernels: k_meta_dense, k_pt_bounce<ST, false> / k_scan / k_pt_shadow<ST> per bounce
//   k_map_fold / k_map_resolve   k_acc_resolve_terms' additions (accum.hip): each slot's terms folded (one thread per slot), then the colours of one
//                        entry's slot range added in sample order, reading and writing the float4 row
//   k_map_flag / k_compact_*   the next layer's list: the entries with add > k0 + cn
//   k_map_finish         count += add, and k_acc_mean's rgb and noise with the pixel's own N, for every pixel of the call's buckets
// k_map_black answers maxTraceDepth < 0.  Launches per layer and batch do not depend on how many distinct values the map holds.
// A call with a second state (frayhip_render_components_map: SampleMapCall::accumIndirect) runs the same layers, lists and tracing and, chosen at
// run time, k_map_fold_split / k_map_resolve_split / k_map_finish_split / k_map_black_split in place of the four above: term 0 of a sample into the
// direct row, the fold of its other terms (kept in the slot's term-1 planes, so the workspace is the same) into the indirect one.
#include "samplemap.hpp"
#include "dev_compact.hpp"
#include "render_impl.hpp"

#ifndef FRAY_ST
#error "compile with -DFRAY_ST=0..5, 8 or 9"
#endif

namespace {

// What the host reads back: the compacted list's length, a batch's slot count, and what k_map_init / k_map_finish found
struct MapHead {
    int count;                    // k_compact_scan: the new list's length
    int slots;                    // k_compact_scan over c_i: the batch's slots
    int bad;                      // a pixel of the call's buckets with add < 0, count < 0 or count + add > 2^24
    int addMax;
    int cntMaxInv, cntMax;        // 2^24 - the smallest count after the call, and the largest
    unsigned long long samples;   // sum of add
    unsigned long long pixels;    // pixels of the call's buckets inside the frame
};

// One batch: entries p0 .. p0 + np - 1 of the layer's list, layer offset k0, at most cn samples of each; off[0 .. np] are the entries' first slots
struct MapBatch {
    const int* list;
    int p0, np, k0, cn;
    const int32_t* add;
    const int32_t* count;
    const int* off;
    const int* slotEntry;
};

FD size_t map_pixel(const DFrame& F, int item, int& x, int& y)
{
    item_pixel(F, item, x, y);
    return (size_t)y * F.W + x;
}
FD int map_take(const DFrame& F, const MapBatch& B, int i)
{
    int x, y;
    return min(B.cn, B.add[map_pixel(F, B.list[B.p0 + i], x, y)] - B.k0);
}

static __global__ __launch_bounds__(256) void k_map_init(DFrame F, int nItems, const int32_t* __restrict__ add, const int32_t* __restrict__ count,
                                                         int* __restrict__ list, unsigned char* __restrict__ flag, MapHead* head)
{
    __shared__ int sMax, sBad;
    __shared__ unsigned long long sSum, sPix;
    if (threadIdx.x == 0) { sMax = 0; sBad = 0; sSum = 0; sPix = 0; }
    __syncthreads();
    int tMax = 0, tBad = 0;
    unsigned long long tSum = 0, tPix = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nItems; i += gridDim.x * blockDim.x) {
        int x, y;
        list[i] = i;
        unsigned char f = 0;
        if (item_pixel(F, i, x, y)) {
            const size_t p = (size_t)y * F.W + x;
            const int a = add[p], n = count[p];
            tPix++;
            if (a < 0 || n < 0 || (long long)n + a > (long long)frayhip_detail::kMapMaxSamples) tBad = 1;
            else if (a > 0) { f = 1; tMax = max(tMax, a); tSum += (unsigned long long)a; }
        }
        flag[i] = f;
    }
    if (tBad) atomicOr(&sBad, 1);
    if (tMax) atomicMax(&sMax, tMax);
    if (tSum) atomicAdd(&sSum, tSum);
    if (tPix) atomicAdd(&sPix, tPix);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sBad) atomicOr(&head->bad, 1);
        if (sMax) atomicMax(&head->addMax, sMax);
        if (sSum) atomicAdd(&head->samples, sSum);
        if (sPix) atomicAdd(&head->pixels, sPix);
    }
}

// The next layer's flags: the entries of the current list that go on past offset k1
static __global__ __launch_bounds__(256) void k_map_flag(DFrame F, const int* __restrict__ list, int n, int k1, const int32_t* __restrict__ add,
                                                         unsigned char* __restrict__ flag)
{
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        int x, y;
        flag[j] = add[map_pixel(F, list[j], x, y)] > k1 ? 1 : 0;
    }
}

// ---- exclusive scan of c_i over a batch's entries, in k_compact_*'s tiles: the tiles' sums, k_compact_scan over them (its total is the batch's
// slot count), then every tile writes its entries' offsets; the tile that holds the last entry also writes off[np]
static __global__ __launch_bounds__(256) void k_map_count(DFrame F, MapBatch B, int* __restrict__ tileCount)
{
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const int base = blockIdx.x * kTile + threadIdx.x * kPerThread;
    int c = 0;
    for (int k = 0; k < kPerThread; k++) if (base + k < B.np) c += map_take(F, B, base + k);
    if (c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0) tileCount[blockIdx.x] = total;
}

static __global__ __launch_bounds__(256) void k_map_offsets(DFrame F, MapBatch B, const int* __restrict__ tileOffset, int* __restrict__ off)
{
    __shared__ int lds[256];
    const int base = blockIdx.x * kTile + threadIdx.x * kPerThread;
    int ck[kPerThread], c = 0;
    for (int k = 0; k < kPerThread; k++) { ck[k] = base + k < B.np ? map_take(F, B, base + k) : 0; c += ck[k]; }
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
        if (base + k < B.np) {
            off[base + k] = o;
            o += ck[k];
            if (base + k == B.np - 1) off[B.np] = o;
        }
}

// slotEntry[slot] = the entry whose slot range holds it: the largest i < np with off[i] <= slot (every entry has at least one slot)
static __global__ __launch_bounds__(256) void k_map_expand(const int* __restrict__ off, int np, uint32_t total, int* __restrict__ slotEntry)
{
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < total; slot += gridDim.x * blockDim.x) {
        int lo = 0, hi = np;
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((uint32_t)off[mid] <= slot) lo = mid; else hi = mid;
        }
        slotEntry[slot] = lo;
    }
}

// The (pixel, sample) of a slot: its entry's pixel, and the pixel's count before the call + the layer's offset + the slot's place in the entry's range
FD void map_slot(const DFrame& F, const MapBatch& B, uint32_t slot, int& x, int& y, uint32_t& sample)
{
    const int i = B.slotEntry[slot];
    const size_t p = map_pixel(F, B.list[B.p0 + i], x, y);
    sample = (uint32_t)(B.count[p] + B.k0) + (slot - (uint32_t)B.off[i]);
}

// k_seed_list (adaptive_variant.hip) with the slot's (pixel, sample) looked up: x397[slot], k_seed's recurrence, FRAY_SEED_CHAINS chains per lane
static __global__ __launch_bounds__(256) void k_seed_map(DFrame F, MapBatch B, uint32_t total, uint32_t* __restrict__ x397)
{
    constexpr int NC = FRAY_SEED_CHAINS;
    const uint32_t groups = (total + NC - 1u) / NC;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
        uint32_t b[NC], slot[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) {
            slot[k] = q + (uint32_t)k * groups;
            b[k] = 0;
            if (slot[k] < total) {
                int x, y;
                uint32_t s;
                map_slot(F, B, slot[k], x, y, s);
                b[k] = sample_seed(F.seed, (uint32_t)y * (uint32_t)F.W + (uint32_t)x, s);
            }
        }
#pragma unroll 1
        for (uint32_t i = 1; i <= 397; i++) {
#pragma unroll
            for (int k = 0; k < NC; k++) b[k] = mt_lcg(b[k], i);
        }
#pragma unroll
        for (int k = 0; k < NC; k++) if (slot[k] < total) x397[slot[k]] = b[k];
    }
}

// k_pt_init_list (adaptive_variant.hip) with the slot's (pixel, sample) looked up.  Every slot holds a path, and every sample counts in `samples`,
// with or without the counting variant.
template <int ST>
static __global__ __launch_bounds__(256) void k_pt_init_map(DCamera C, DFrame F, MapBatch B, uint32_t total, PathQueue Q, unsigned short* __restrict__ termCount,
                                                            const uint32_t* __restrict__ x397, DStats* st)
{
    Cnt c = zero_cnt();
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < total; slot += gridDim.x * blockDim.x) {
        int x, y;
        uint32_t s;
        map_slot(F, B, slot, x, y, s);
        PathState ps;
        const uint32_t p = (uint32_t)y * (uint32_t)F.W + (uint32_t)x;
        ps.rnd = mt_seed_with(sample_seed(F.seed, p, s), x397[slot]);
        ps.tab = ps.rnd;
        float ox = rng_float(ps.rnd), oy = rng_float(ps.rnd);           // gi: always jittered (main.cpp:351-353)
        double fx = (double)((float)x + ox), fy = (double)((float)y + oy);
        if (C.dof) dof_ray(C, fx, fy, ps.tab, ps.o, ps.d); else screen_ray(C, fx, fy, ps.o, ps.d);
        ps.pm = c3(1, 1, 1);
        ps.slot = slot;
        ps.depth = 0;
        ps.flags = 0;
        c.samples++;
        path_store<FRAY_SORT && sort_variant(ST)>(Q, slot, ps, ray_sort_class<ST>(ps.d, 0u));
        termCount[slot] = 0;
    }
    if (ST & 1) flush_stats(st, c);
    else if (c.samples) atomicAdd(&st->samples, c.samples);
}

// accum.hip's acc_lum and acc_add: ((r + g) + b) / 3.0f; sum + c per channel, then m2 + l * l (no contraction: -ffp-contract=off)
FD float map_lum(C3 c) { return ((c.r + c.g) + c.b) / 3.0f; }
FD void map_add(float4& row, C3 c)
{
    const C3 a = c3(row.x, row.y, row.z) + c;
    const float l = map_lum(c);
    row.x = a.r; row.y = a.g; row.z = a.b;
    row.w = row.w + l * l;
}

// The first half of k_acc_resolve_terms' arithmetic, one thread per slot so that a wave reads each term plane in one piece: the sample's terms
// folded innermost first (the same additions in the same order), the colour left in the slot's term 0
static __global__ __launch_bounds__(256) void k_map_fold(uint32_t total, TermBuf TB)
{
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < total; slot += gridDim.x * blockDim.x) {
        const int n = (int)TB.n[slot];
        C3 result = c3(0, 0, 0);
        if (n <= 8) {
            // up to eight terms: every load issued before the first addition, as k_pt_resolve_terms does
            float tr[8], tg[8], tb[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                tr[k] = tg[k] = tb[k] = 0.0f;
                if (k < n) {
                    const size_t q = (size_t)k * 3 * TB.nPaths + slot;
                    tr[k] = TB.t[q]; tg[k] = TB.t[q + TB.nPaths]; tb[k] = TB.t[q + 2 * (size_t)TB.nPaths];
                }
            }
#pragma unroll
            for (int k = 7; k >= 0; k--)
                if (k < n) result = c3(tr[k], tg[k], tb[k]) + result;
        } else {
            for (int k = n - 1; k >= 0; k--) {
                const size_t q = (size_t)k * 3 * TB.nPaths + slot;
                result = c3(TB.t[q], TB.t[q + TB.nPaths], TB.t[q + 2 * (size_t)TB.nPaths]) + result;
            }
        }
        TB.t[slot] = result.r; TB.t[slot + TB.nPaths] = result.g; TB.t[slot + 2 * (size_t)TB.nPaths] = result.b;
    }
}

// The second half, per entry: the row is read (a pixel that holds no sample starts at (0, 0, 0, 0)), the folded colours of the entry's slot range are
// added in sample order (acc_add), and the row is written back.  A thread walks consecutive addresses, so its cache lines serve the whole walk.
static __global__ __launch_bounds__(256) void k_map_resolve(DFrame F, MapBatch B, TermBuf TB, float4* __restrict__ accum)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B.np; i += gridDim.x * blockDim.x) {
        int x, y;
        const size_t p = map_pixel(F, B.list[B.p0 + i], x, y);
        float4 row = B.count[p] + B.k0 == 0 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : accum[p];
        const uint32_t s0 = (uint32_t)B.off[i], s1 = (uint32_t)B.off[i + 1];
        for (uint32_t slot = s0; slot < s1; slot++)
            map_add(row, c3(TB.t[slot], TB.t[slot + TB.nPaths], TB.t[slot + 2 * (size_t)TB.nPaths]));
        accum[p] = row;
    }
}

// ---- two states (frayhip_render_components_map): a sample's term 0 is its direct light, the fold of its terms 1 .. n-1 its indirect light
// k_acc_resolve_terms_split's first half, one thread per slot: term 0 stays where it is, as stored; the fold of the others, begun at (0, 0, 0) and
// innermost first, goes into the slot's term-1 planes (a traced call has nBounce >= 2, so they exist; in the loop form term 1 is the last one read,
// before it is overwritten).  A wave reads and writes each plane in one piece, as k_map_fold does.
static __global__ __launch_bounds__(256) void k_map_fold_split(uint32_t total, TermBuf TB)
{
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < total; slot += gridDim.x * blockDim.x) {
        const int n = (int)TB.n[slot];
        C3 result = c3(0, 0, 0);
        if (n <= 8) {
            // up to eight terms: every load issued before the first addition
            float tr[8], tg[8], tb[8];
#pragma unroll
            for (int k = 1; k < 8; k++) {
                tr[k] = tg[k] = tb[k] = 0.0f;
                if (k < n) {
                    const size_t q = (size_t)k * 3 * TB.nPaths + slot;
                    tr[k] = TB.t[q]; tg[k] = TB.t[q + TB.nPaths]; tb[k] = TB.t[q + 2 * (size_t)TB.nPaths];
                }
            }
#pragma unroll
            for (int k = 7; k >= 1; k--)
                if (k < n) result = c3(tr[k], tg[k], tb[k]) + result;
        } else {
            for (int k = n - 1; k >= 1; k--) {
                const size_t q = (size_t)k * 3 * TB.nPaths + slot;
                result = c3(TB.t[q], TB.t[q + TB.nPaths], TB.t[q + 2 * (size_t)TB.nPaths]) + result;
            }
        }
        const size_t q1 = (size_t)3 * TB.nPaths + slot;
        TB.t[q1] = result.r; TB.t[q1 + TB.nPaths] = result.g; TB.t[q1 + 2 * (size_t)TB.nPaths] = result.b;
        if (n == 0) { TB.t[slot] = 0.0f; TB.t[slot + TB.nPaths] = 0.0f; TB.t[slot + 2 * (size_t)TB.nPaths] = 0.0f; }          // no term: direct light (0, 0, 0)
    }
}

// The second half, per entry, for both rows: term 0 of the entry's slots into the direct row, the fold in their term-1 planes into the indirect one
static __global__ __launch_bounds__(256) void k_map_resolve_split(DFrame F, MapBatch B, TermBuf TB, float4* __restrict__ direct, float4* __restrict__ indirect)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B.np; i += gridDim.x * blockDim.x) {
        int x, y;
        const size_t p = map_pixel(F, B.list[B.p0 + i], x, y);
        const bool fresh = B.count[p] + B.k0 == 0;
        float4 rowD = fresh ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : direct[p];
        float4 rowI = fresh ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : indirect[p];
        const uint32_t s0 = (uint32_t)B.off[i], s1 = (uint32_t)B.off[i + 1];
        const size_t plane1 = (size_t)3 * TB.nPaths;
        // one walk per component (the rows do not depend on each other): a thread then has three address streams in flight, as in k_map_resolve,
        // and its cache lines still serve the whole walk; with all six at once they did not (33 M slots: 1.53 ms in one walk, 0.99 ms in two; the
        // single-state resolve takes 0.52 ms)
        for (uint32_t slot = s0; slot < s1; slot++)
            map_add(rowD, c3(TB.t[slot], TB.t[slot + TB.nPaths], TB.t[slot + 2 * (size_t)TB.nPaths]));
        for (uint32_t slot = s0; slot < s1; slot++)
            map_add(rowI, c3(TB.t[plane1 + slot], TB.t[plane1 + slot + TB.nPaths], TB.t[plane1 + slot + 2 * (size_t)TB.nPaths]));
        direct[p] = rowD;
        indirect[p] = rowI;
    }
}

// k_map_black for two states: one +0 into both rows, the samples counted once
static __global__ __launch_bounds__(256) void k_map_black_split(DFrame F, int nItems, const int32_t* __restrict__ add, const int32_t* __restrict__ count,
                                                                float4* __restrict__ direct, float4* __restrict__ indirect, DStats* st)
{
    unsigned long long n = 0;
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        const size_t p = (size_t)y * F.W + x;
        const int a = add[p];
        if (a <= 0) continue;
        const bool fresh = count[p] == 0;
        float4 rowD = fresh ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : direct[p];
        float4 rowI = fresh ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : indirect[p];
        map_add(rowD, c3(0, 0, 0));
        map_add(rowI, c3(0, 0, 0));
        direct[p] = rowD;
        indirect[p] = rowI;
        n += (unsigned long long)a;
    }
    if (n) atomicAdd(&st->samples, n);
}

// k_map_finish's rgb and noise of one state's row at N >= 1 samples (k_acc_mean's arithmetic); either output may be null
FD void map_mean(const float4* __restrict__ accum, size_t p, int n, float* __restrict__ rgb, float* __restrict__ noise)
{
    if (!rgb && !noise) return;
    const float4 row = accum[p];
    const C3 m = c3(row.x, row.y, row.z) / (float)n;
    if (rgb) { rgb[p * 3] = m.r; rgb[p * 3 + 1] = m.g; rgb[p * 3 + 2] = m.b; }
    if (noise) {
        const float lbar = map_lum(m);
        const float v = fmaxf(0.0f, row.w / (float)n - lbar * lbar);
        noise[p] = n >= 2 ? v / (float)(n - 1) : lbar * lbar;
    }
}

// k_map_finish for two states: count += add once, then each component's rgb and noise from its own row and the pixel's N; all four outputs optional
static __global__ __launch_bounds__(256) void k_map_finish_split(DFrame F, int nItems, const int32_t* __restrict__ add, int32_t* __restrict__ count,
                                                                 const float4* __restrict__ direct, const float4* __restrict__ indirect,
                                                                 float* __restrict__ rgbD, float* __restrict__ rgbI, float* __restrict__ noiseD,
                                                                 float* __restrict__ noiseI, MapHead* head)
{
    __shared__ int sMaxInv, sMax;
    if (threadIdx.x == 0) { sMaxInv = 0; sMax = 0; }
    __syncthreads();
    int tMax = 0, tMaxInv = 0;
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        const size_t p = (size_t)y * F.W + x;
        const int a = add[p], n = count[p] + a;
        if (a > 0) count[p] = n;
        tMax = max(tMax, n);
        tMaxInv = max(tMaxInv, frayhip_detail::kMapMaxSamples - n);
        if (n == 0) {
            if (rgbD) { rgbD[p * 3] = 0.0f; rgbD[p * 3 + 1] = 0.0f; rgbD[p * 3 + 2] = 0.0f; }
            if (rgbI) { rgbI[p * 3] = 0.0f; rgbI[p * 3 + 1] = 0.0f; rgbI[p * 3 + 2] = 0.0f; }
            if (noiseD) noiseD[p] = 0.0f;
            if (noiseI) noiseI[p] = 0.0f;
            continue;
        }
        map_mean(direct, p, n, rgbD, noiseD);
        map_mean(indirect, p, n, rgbI, noiseI);
    }
    if (tMax) atomicMax(&sMax, tMax);
    if (tMaxInv) atomicMax(&sMaxInv, tMaxInv);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sMax) atomicMax(&head->cntMax, sMax);
        if (sMaxInv) atomicMax(&head->cntMaxInv, sMaxInv);
    }
}

// maxTraceDepth < 0: pathtrace() returns black before it looks at the scene.  k_acc_black's arithmetic for the pixels the map names: one addition
// of +0 (the later ones change nothing), the samples counted.
static __global__ __launch_bounds__(256) void k_map_black(DFrame F, int nItems, const int32_t* __restrict__ add, const int32_t* __restrict__ count,
                                                          float4* __restrict__ accum, DStats* st)
{
    unsigned long long n = 0;
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        const size_t p = (size_t)y * F.W + x;
        const int a = add[p];
        if (a <= 0) continue;
        float4 row = count[p] == 0 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : accum[p];
        map_add(row, c3(0, 0, 0));
        accum[p] = row;
        n += (unsigned long long)a;
    }
    if (n) atomicAdd(&st->samples, n);
}

// The end of a call, for every pixel of its buckets: count += add, and k_acc_mean's rgb and noise (accum.hip) with the pixel's own N; a pixel
// that holds no sample knows nothing: rgb (0, 0, 0), noise 0.  The smallest and the largest N go to the head.
static __global__ __launch_bounds__(256) void k_map_finish(DFrame F, int nItems, const int32_t* __restrict__ add, int32_t* __restrict__ count,
                                                           const float4* __restrict__ accum, float* __restrict__ rgb, float* __restrict__ noise, MapHead* head)
{
    __shared__ int sMaxInv, sMax;
    if (threadIdx.x == 0) { sMaxInv = 0; sMax = 0; }
    __syncthreads();
    int tMax = 0, tMaxInv = 0;
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        const size_t p = (size_t)y * F.W + x;
        const int a = add[p], n = count[p] + a;
        if (a > 0) count[p] = n;
        tMax = max(tMax, n);
        tMaxInv = max(tMaxInv, frayhip_detail::kMapMaxSamples - n);
        if (!rgb && !noise) continue;
        if (n == 0) {
            if (rgb) { rgb[p * 3] = 0.0f; rgb[p * 3 + 1] = 0.0f; rgb[p * 3 + 2] = 0.0f; }
            if (noise) noise[p] = 0.0f;
            continue;
        }
        const float4 row = accum[p];
        const C3 m = c3(row.x, row.y, row.z) / (float)n;          // the frame's own division
        if (rgb) { rgb[p * 3] = m.r; rgb[p * 3 + 1] = m.g; rgb[p * 3 + 2] = m.b; }
        if (noise) {
            const float lbar = map_lum(m);
            const float v = fmaxf(0.0f, row.w / (float)n - lbar * lbar);
            noise[p] = n >= 2 ? v / (float)(n - 1) : lbar * lbar;
        }
    }
    if (tMax) atomicMax(&sMax, tMax);
    if (tMaxInv) atomicMax(&sMaxInv, tMaxInv);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sMax) atomicMax(&head->cntMax, sMax);
        if (sMaxInv) atomicMax(&head->cntMaxInv, sMaxInv);
    }
}

}  // namespace

namespace frayhip_detail {

// One call on ONE stream (the caller's), adaptive_impl's rule.  Per layer, batches of list entries whose slots fit the scene's work budget; the
// host reads the list's length once per layer and a batch's slot count once per batch.
template <int ST>
int samplemap_impl(frayhip_scene* sc, SampleMapCall& q, hipStream_t stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const frayhip_settings& set = sc->settings;
    const DFrame F = frame_record(sc, q.bucketFirst, q.bucketStride, q.seed);
    const int nItems = F.nBuckets * 2304;
    const DScene S = frame_scene(sc);
    const DCamera C = camera_begin_frame(sc->camera, F.W, F.H);

    // a map call is a frame: the last frame's figures are its own (it runs no contracted kernel and no speculative fan)
    sc->lastContracted = 0;
    for (int k = 0; k < 4; k++) sc->lastFans[k] = 0;
    q.samples = 0;
    q.countMin = q.countMax = 0;
    q.badPlanes = false;
    const bool pair = q.accumIndirect != nullptr;          // a component call: the split fold, resolve and finish
    const char* who = pair ? "frayhip_render_components_map" : "frayhip_render_samples_map";
    HIP_TRY(hipMemsetAsync(sc->d_stats, 0, kStatsBytes, stream));
    HIP_TRY(hipEventRecord(sc->evA, stream));
    size_t nTraceEvents = 0, nShadowEvents = 0;

    if (nItems > 0) {
        const bool alone = (ST & 2) != 0;
        const bool black = set.maxTraceDepth < 0;
        const int nBounce = set.maxTraceDepth + 2;
        const size_t termBytes = (size_t)std::max(nBounce, 0) * 12 + 2;
        const int nTiles = (nItems + kTile - 1) / kTile;
        // the head; per work item: two lists and the offsets (12 B + one more offset), a flag; per tile: count and offset
        const size_t stateBytes = 256 + 2 * r256((size_t)nItems * 4) + r256((size_t)nItems * 4 + 4) + r256((size_t)nItems) + 2 * r256((size_t)nTiles * 4);
        MapHead* head = nullptr;
        int* list[2] = {nullptr, nullptr};
        int *off = nullptr, *tileCount = nullptr, *tileOffset = nullptr;
        unsigned char* flag = nullptr;
        Carve work{nullptr};
        auto carve_state = [&] {
            work = Carve{(unsigned char*)sc->d_work};
            head = (MapHead*)work.take(256);
            list[0] = (int*)work.take((size_t)nItems * 4);
            list[1] = (int*)work.take((size_t)nItems * 4);
            off = (int*)work.take((size_t)nItems * 4 + 4);
            flag = work.take((size_t)nItems);
            tileCount = (int*)work.take((size_t)nTiles * 4);
            tileOffset = (int*)work.take((size_t)nTiles * 4);
        };
        MapHead h{};
        auto read_head = [&]() -> int {
            HIP_TRY(hipMemcpyAsync(&h, head, sizeof h, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            return FRAYHIP_OK;
        };
        // the list's new length, read back once per compaction
        int cur = 0;
        auto compact = [&](int n, int& out) -> int {
            const int tiles = (n + kTile - 1) / kTile;
            hipLaunchKernelGGL(k_compact_count, dim3(tiles), dim3(256), 0, stream, (const unsigned char*)flag, n, tileCount);
            hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, stream, (const int*)tileCount, tiles, tileOffset, &head->count);
            hipLaunchKernelGGL(k_compact_write, dim3(tiles), dim3(256), 0, stream, (const int*)list[cur], (const unsigned char*)flag, n, (const int*)tileOffset, list[cur ^ 1]);
            if (const int rc = read_head()) return rc;
            out = h.count;
            cur ^= 1;
            return FRAYHIP_OK;
        };
        // the planes' check and the first list: every pixel of the call's buckets with add > 0
        int nActive = 0;
        auto first_list = [&]() -> int {
            cur = 0;
            HIP_TRY(hipMemsetAsync(head, 0, sizeof(MapHead), stream));
            hipLaunchKernelGGL(k_map_init, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, q.add, (const int32_t*)q.count, list[0], flag, head);
            return compact(nItems, nActive);
        };
        {
            const int rc = ensure_work_or_shrink(sc, stateBytes, false);
            if (rc) return rc;
        }
        carve_state();
        if (const int rc = first_list()) return rc;
        if (h.bad) { q.badPlanes = true; return FRAYHIP_E_ARG; }          // nothing has been written to the caller's buffers
        q.samples = h.samples;
        const int addMax = h.addMax;

        if (black && pair) {
            hipLaunchKernelGGL(k_map_black_split, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, q.add, (const int32_t*)q.count, (float4*)q.accum,
                               (float4*)q.accumIndirect, sc->d_stats);
        } else if (black) {
            hipLaunchKernelGGL(k_map_black, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, q.add, (const int32_t*)q.count, (float4*)q.accum, sc->d_stats);
        } else if (nActive > 0) {
            int maxLayer = addMax;
            if (q.sppChunk > 0) maxLayer = std::min(maxLayer, q.sppChunk);
            size_t slots = 0, nQueue = 0;
            for (;;) {          // planned again with half the budget when the allocation fails
                const size_t wb = work_budget(sc);
                const size_t budget = wb > stateBytes + (64u << 20) ? wb - stateBytes : (64u << 20);
                slots = std::min<size_t>(std::max<size_t>(budget / (244 + termBytes), 64), (size_t)1 << 30);
                slots = std::min<size_t>(slots, (size_t)nActive * (size_t)maxLayer);
                nQueue = slots + (size_t)bounce_grid(slots, alone) * 4 * 128;          // per-wave segments round their share up to a multiple of 64
                const size_t bytes = stateBytes + 2 * queue_bytes(nQueue) + shadow_bytes(nQueue) + 2 * r256(slots * 4) + r256(slots * (size_t)nBounce * 12) + r256(slots * 2);
                const size_t held = sc->work_bytes;
                const int rc = ensure_work_or_shrink(sc, bytes, q.sppChunk <= 0 && slots > 64);
                if (rc == FRAYHIP_RETRY_SMALLER) continue;
                if (rc) return rc;
                if (sc->work_bytes != held) {          // the workspace was allocated anew (ensure_work, maybe at the old address): the list is made again
                    carve_state();
                    if (const int rc2 = first_list()) return rc2;
                }
                break;
            }
            PathQueue Q[2];
            ShadowQueue SQ;
            work.p = carve_queue(work.p, nQueue, Q[0]);
            work.p = carve_queue(work.p, nQueue, Q[1]);
            work.p = carve_shadow(work.p, nQueue, SQ);
            uint32_t* x397 = (uint32_t*)work.take(slots * 4);
            int* slotEntry = (int*)work.take(slots * 4);
            float* terms = (float*)work.take(slots * (size_t)nBounce * 12);
            unsigned short* termCount = (unsigned short*)work.take(slots * 2);
            QMeta* meta = sc->d_qmeta;
            const TermBuf TB{terms, termCount, (uint32_t)slots, 0};

            for (int k0 = 0; nActive > 0;) {
                const int np = (int)std::min<size_t>((size_t)nActive, slots);
                int cn = (int)std::min<size_t>((size_t)(addMax - k0), std::max<size_t>(1, slots / (size_t)np));
                if (q.sppChunk > 0) cn = std::min(cn, q.sppChunk);
                for (int p0 = 0; p0 < nActive; p0 += np) {
                    const int mp = std::min(np, nActive - p0);
                    const MapBatch B{list[cur], p0, mp, k0, cn, q.add, (const int32_t*)q.count, off, slotEntry};
                    const int tiles = (mp + kTile - 1) / kTile;
                    hipLaunchKernelGGL(k_map_count, dim3(tiles), dim3(256), 0, stream, F, B, tileCount);
                    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, stream, (const int*)tileCount, tiles, tileOffset, &head->slots);
                    hipLaunchKernelGGL(k_map_offsets, dim3(tiles), dim3(256), 0, stream, F, B, (const int*)tileOffset, off);
                    if (const int rc = read_head()) return rc;
                    const size_t m = (size_t)h.slots;
                    if (m < (size_t)mp || m > (size_t)mp * (size_t)cn || m > slots) {
                        set_error(std::string(who) + ": a batch's slot count is out of range (the add plane changed during the call?)");
                        return FRAYHIP_E_ARG;
                    }
                    hipLaunchKernelGGL(k_map_expand, dim3(grid_for(m)), dim3(256), 0, stream, (const int*)off, mp, (uint32_t)m, slotEntry);
                    hipLaunchKernelGGL(k_seed_map, dim3(seed_grid((m + FRAY_SEED_CHAINS - 1) / FRAY_SEED_CHAINS)), dim3(256), 0, stream, F, B, (uint32_t)m, x397);
                    hipLaunchKernelGGL(k_meta_dense, dim3(1), dim3(64), 0, stream, meta, (uint32_t)m);
                    hipLaunchKernelGGL(k_pt_init_map<ST>, dim3(grid_for(m)), dim3(256), 0, stream, C, F, B, (uint32_t)m, Q[0], termCount, (const uint32_t*)x397, sc->d_stats);
                    if (const int rc = pt_bounces<ST>(sc, S, Q, SQ, TB, nBounce, bounce_grid(m, alone), stream, nTraceEvents, nShadowEvents)) return rc;
                    if (pair) {
                        hipLaunchKernelGGL(k_map_fold_split, dim3(grid_for(m)), dim3(256), 0, stream, (uint32_t)m, TB);
                        hipLaunchKernelGGL(k_map_resolve_split, dim3(grid_for((size_t)mp)), dim3(256), 0, stream, F, B, TB, (float4*)q.accum, (float4*)q.accumIndirect);
                    } else {
                        hipLaunchKernelGGL(k_map_fold, dim3(grid_for(m)), dim3(256), 0, stream, (uint32_t)m, TB);
                        hipLaunchKernelGGL(k_map_resolve, dim3(grid_for((size_t)mp)), dim3(256), 0, stream, F, B, TB, (float4*)q.accum);
                    }
                }
                k0 += cn;
                if (k0 >= addMax) break;
                hipLaunchKernelGGL(k_map_flag, dim3(grid_for((size_t)nActive)), dim3(256), 0, stream, F, (const int*)list[cur], nActive, k0, q.add, flag);
                if (const int rc = compact(nActive, nActive)) return rc;
            }
        }
        if (pair)
            hipLaunchKernelGGL(k_map_finish_split, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, q.add, q.count, (const float4*)q.accum,
                               (const float4*)q.accumIndirect, q.rgb, q.rgbIndirect, q.noise, q.noiseIndirect, head);
        else
            hipLaunchKernelGGL(k_map_finish, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, q.add, q.count, (const float4*)q.accum, q.rgb, q.noise, head);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(sc->evB, stream));
        if (const int rc = read_head()) return rc;
        if (h.pixels) { q.countMin = kMapMaxSamples - h.cntMaxInv; q.countMax = h.cntMax; }
    } else {
        HIP_TRY(hipEventRecord(sc->evB, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    DStats dsv[2];
    HIP_TRY(hipMemcpy(dsv, sc->d_stats, sizeof dsv, hipMemcpyDeviceToHost));
    if (dsv[0].rngOverflow || dsv[1].rngOverflow) {
        set_error(std::string(who) + ": a camera sample left the supported envelope (a generator past 227 words; a CsgOp operand with more "
                  "intersections than the device path holds)");
        return FRAYHIP_E_UNSUPPORTED;
    }
    if (st) *st = finish_stats(sc, dsv, 2, nTraceEvents, nShadowEvents, t0);
    return FRAYHIP_OK;
}

template int samplemap_impl<FRAY_ST>(frayhip_scene*, SampleMapCall&, hipStream_t, frayhip_stats*);

}  // namespace frayhip_detail
