// C ABI, split temporal accumulation (include/frayhip.h "split temporal accumulation"): frayhip_temporal_accumulate_split,
// frayhip_temporal_accumulate_split_adaptive and their _device entries.
// temporal.hip's stage for two signals of one frame -- a frame's direct and indirect light (frayhip_render_components) -- with one history of
// five float4 rows a pixel: the projection, the footprint and the surface tests run once, each counted tap is read once, and everything per
// component is temporal.hip's expression on the other component's inputs, so each group of outputs equals frayhip_temporal_accumulate[_motion]'s
// for that component bit for bit.  The Makefile builds this object by temporal.o's rule (-ffp-contract=off, correctly rounded divide and sqrt).
//
//   k_tp_accumulate_split  per pixel: both signals, one projection into the previous view, four taps of five float4 rows each, the seven history
//                          sums once per component, the blend with each component's max_history and alpha_min; writes the five history rows,
//                          both signals, and each component's temporal variance where its N >= its variance_history.  <MOTION> as
//                          k_tp_accumulate's.  <MOTION, ADAPTIVE>: one change frame per component (change.hip) shortens that component's
//                          history per pixel, by k_tp_accumulate<MOTION, true>'s three cases; the two components may take different cases
//                          in one pixel.  <MOTION, false> are the two kernels as they were
//   k_tp_variance_split    per pixel with N_D < variance_history_D or N_I < variance_history_I: the 7x7 window of the finished history, its
//                          surface tests once, the moments' sums per component; the 16x16 block stages rows 1, 2 and 4 of the 22x22 texels as
//                          three planes of float4; a block without such a pixel stages nothing
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "entry_support.hpp"
#include "temporal_common.hpp"

#define FRAY_TPS_ROWS 5                  // FRAYHIP_HISTORY_SPLIT_CHANNELS / 4

struct TemporalSplitCall {
    int W, H;
    const float* rgb[2];        // 0: direct, 1: indirect, here and below
    const float* feat;
    const float4* motion;       // k_tp_accumulate_split<true> only: two rows a pixel
    const float4* histIn;       // null: first frame
    float4* histOut;
    float* signal[2];
    float* variance[2];
    frayhip_view view;          // read only with histIn
    int demodulate, varianceHistory[2];
    float maxHistory[2], alphaMin[2], filmOffset, planeTolerance, normalMinDot;
    const float* change[2];     // k_tp_accumulate_split<MOTION, true> only: one float a pixel per component
};

// One component's history sums over the counted taps, and k_tp_accumulate's steps on them
struct TpSums {
    float r = 0.0f, g = 0.0f, b = 0.0f, n = 0.0f, m1 = 0.0f, m2 = 0.0f;
    __device__ __forceinline__ void tap(float w, float qr, float qg, float qb, float qn, float q1, float q2)
    {
        r += w * qr; g += w * qg; b += w * qb; n += w * qn;
        m1 += w * q1; m2 += w * q2;
    }
};

struct TpBlend { float r, g, b, N, m1, m2; };

static __device__ __forceinline__ TpBlend tp_blend(TpSums h, float sb, float cr, float cg, float cb, float maxHistory, float alphaMin)
{
    const float l = tp_lum(cr, cg, cb);
    const float l2 = l * l;
    TpBlend o{cr, cg, cb, 1.0f, l, l2};
    if (sb > 0.0f) {
        h.r = h.r / sb; h.g = h.g / sb; h.b = h.b / sb; h.n = h.n / sb; h.m1 = h.m1 / sb; h.m2 = h.m2 / sb;
        o.N = fminf(h.n + 1.0f, maxHistory);
        const float alpha = fmaxf(alphaMin, 1.0f / o.N);
        o.r = h.r + alpha * (cr - h.r); o.g = h.g + alpha * (cg - h.g); o.b = h.b + alpha * (cb - h.b);
        o.m1 = h.m1 + alpha * (l - h.m1);
        o.m2 = h.m2 + alpha * (l2 - h.m2);
    }
    return o;
}

// tp_blend with a component's change g (0 where no history was fetched): k_tp_accumulate<MOTION, true>'s three cases, each sum and division
// in that kernel's order
static __device__ __forceinline__ TpBlend tp_blend_adaptive(TpSums h, float sb, float cr, float cg, float cb, float g, float maxHistory, float alphaMin)
{
    const float l = tp_lum(cr, cg, cb);
    const float l2 = l * l;
    TpBlend o{cr, cg, cb, 1.0f, l, l2};
    if (!(g < 1.0f)) {
        // changed through and through (1, above 1, NaN): no history, the first-frame values above
    } else if (g > 0.0f) {
        h.r = h.r / sb; h.g = h.g / sb; h.b = h.b / sb; h.n = h.n / sb; h.m1 = h.m1 / sb; h.m2 = h.m2 / sb;
        const float N0 = fminf(h.n + 1.0f, maxHistory);
        const float a0 = fmaxf(alphaMin, 1.0f / N0);
        const float alpha = a0 + g * (1.0f - a0);
        o.N = fminf(N0, 1.0f / alpha);
        o.r = h.r + alpha * (cr - h.r); o.g = h.g + alpha * (cg - h.g); o.b = h.b + alpha * (cb - h.b);
        o.m1 = h.m1 + alpha * (l - h.m1);
        o.m2 = h.m2 + alpha * (l2 - h.m2);
    } else if (sb > 0.0f) {
        h.r = h.r / sb; h.g = h.g / sb; h.b = h.b / sb; h.n = h.n / sb; h.m1 = h.m1 / sb; h.m2 = h.m2 / sb;
        o.N = fminf(h.n + 1.0f, maxHistory);
        const float alpha = fmaxf(alphaMin, 1.0f / o.N);
        o.r = h.r + alpha * (cr - h.r); o.g = h.g + alpha * (cg - h.g); o.b = h.b + alpha * (cb - h.b);
        o.m1 = h.m1 + alpha * (l - h.m1);
        o.m2 = h.m2 + alpha * (l2 - h.m2);
    }
    return o;
}

template <bool MOTION, bool ADAPTIVE>
static __global__ __launch_bounds__(256) void k_tp_accumulate_split(TemporalSplitCall T)
{
    const int W = T.W, H = T.H;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const float* f = T.feat + p * FRAYHIP_FEAT_CHANNELS;
    const float Px = f[0], Py = f[1], Pz = f[2];
    float nx = f[3], ny = f[4], nz = f[5];
    const float nn = nx * nx + ny * ny + nz * nz;
    if (nn > 0.0f) {                       // k_dn_prepare's unit normal
        const float s = sqrtf(nn);
        nx = nx / s; ny = ny / s; nz = nz / s;
    }
    const float* cd = T.rgb[0] + 3 * p;
    const float* ci = T.rgb[1] + 3 * p;
    float dr = cd[0], dg = cd[1], db = cd[2], ir = ci[0], ig = ci[1], ib = ci[2];
    if (T.demodulate) {
        const float a0 = fmaxf(f[6], 1e-3f), a1 = fmaxf(f[7], 1e-3f), a2 = fmaxf(f[8], 1e-3f);
        dr = dr / a0; dg = dg / a1; db = db / a2;
        ir = ir / a0; ig = ig / a1; ib = ib / a2;
    }

    float sb = 0.0f;
    TpSums hd, hi;
    bool miss = nx == 0.0f && ny == 0.0f && nz == 0.0f;
    // what is carried into the previous view: the pixel's own position and unit normal, or where they were (P', n' scaled as the normal is)
    float Qx = Px, Qy = Py, Qz = Pz, mx = nx, my = ny, mz = nz;
    if constexpr (MOTION) {
        const float4 r0 = T.motion[2 * p], r1 = T.motion[2 * p + 1];
        Qx = r0.x; Qy = r0.y; Qz = r0.z;
        mx = r1.x; my = r1.y; mz = r1.z;
        const float mm = mx * mx + my * my + mz * mz;
        if (mm > 0.0f) {
            const float s = sqrtf(mm);
            mx = mx / s; my = my / s; mz = mz / s;
        }
        miss = miss || (mx == 0.0f && my == 0.0f && mz == 0.0f);
    }
    if (T.histIn && !miss) {
        const frayhip_view& V = T.view;
        const float dx = Qx - V.pos[0], dy = Qy - V.pos[1], dz = Qz - V.pos[2];
        const float zc = tp_dot(dx, dy, dz, V.front[0], V.front[1], V.front[2]);
        if (zc > 0.0f) {
            const float xc = tp_dot(dx, dy, dz, V.right[0], V.right[1], V.right[2]);
            const float yc = tp_dot(dx, dy, dz, V.up[0], V.up[1], V.up[2]);
            const float fx = ((xc / zc / V.tan_x + 1.0f) * 0.5f) * (float)W;
            const float fy = ((1.0f - yc / zc / V.tan_y) * 0.5f) * (float)H;
            const float u = fx - T.filmOffset, v = fy - T.filmOffset;
            const float x0f = floorf(u), y0f = floorf(v);
            // a footprint that touches the image (the comparisons are false for a NaN): only then do the floats fit an int
            if (x0f >= -1.0f && x0f <= (float)(W - 1) && y0f >= -1.0f && y0f <= (float)(H - 1)) {
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float tx = u - x0f, ty = v - y0f;
                const float tol = T.planeTolerance * sqrtf(tp_dot(dx, dy, dz, dx, dy, dz));
                for (int j = 0; j < 2; j++) {
                    const int yq = y0 + j;
                    if (yq < 0 || yq >= H) continue;
                    for (int i = 0; i < 2; i++) {
                        const int xq = x0 + i;
                        if (xq < 0 || xq >= W) continue;
                        const float4* hq = T.histIn + ((size_t)yq * W + xq) * FRAY_TPS_ROWS;
                        const float4 q0 = hq[0], q1 = hq[1], q2 = hq[2], q3 = hq[3], q4 = hq[4];
                        if (q2.x == 0.0f && q2.y == 0.0f && q2.z == 0.0f) continue;
                        if (!(tp_dot(mx, my, mz, q2.x, q2.y, q2.z) >= T.normalMinDot)) continue;
                        if (!(fabsf(tp_dot(q1.x - Qx, q1.y - Qy, q1.z - Qz, mx, my, mz)) <= tol)) continue;
                        const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                        sb += b;
                        hd.tap(b, q0.x, q0.y, q0.z, q0.w, q1.w, q2.w);
                        hi.tap(b, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y);
                    }
                }
            }
        }
    }
    TpBlend D, I;
    if constexpr (ADAPTIVE) {
        float gd = 0.0f, gi = 0.0f;        // each component's change, read only where a history was fetched
        if (sb > 0.0f) { gd = T.change[0][p]; gi = T.change[1][p]; }
        D = tp_blend_adaptive(hd, sb, dr, dg, db, gd, T.maxHistory[0], T.alphaMin[0]);
        I = tp_blend_adaptive(hi, sb, ir, ig, ib, gi, T.maxHistory[1], T.alphaMin[1]);
    } else {
        D = tp_blend(hd, sb, dr, dg, db, T.maxHistory[0], T.alphaMin[0]);
        I = tp_blend(hi, sb, ir, ig, ib, T.maxHistory[1], T.alphaMin[1]);
    }
    float4* ho = T.histOut + p * FRAY_TPS_ROWS;
    ho[0] = make_float4(D.r, D.g, D.b, D.N);
    ho[1] = make_float4(Px, Py, Pz, D.m1);
    ho[2] = make_float4(nx, ny, nz, D.m2);
    ho[3] = make_float4(I.r, I.g, I.b, I.N);
    ho[4] = make_float4(I.m1, I.m2, 0.0f, 0.0f);
    float* sd = T.signal[0] + 3 * p;
    sd[0] = D.r; sd[1] = D.g; sd[2] = D.b;
    float* si = T.signal[1] + 3 * p;
    si[0] = I.r; si[1] = I.g; si[2] = I.b;
    if (D.N >= (float)T.varianceHistory[0]) T.variance[0][p] = fmaxf(0.0f, D.m2 - D.m1 * D.m1);
    if (I.N >= (float)T.varianceHistory[1]) T.variance[1][p] = fmaxf(0.0f, I.m2 - I.m1 * I.m1);
}

// A 16x16 block and the 22x22 texels its 7x7 windows reach: rows 1, 2 and 4 of the history, one plane of float4 each, 48 bytes a texel,
// 23232 bytes of LDS
#define FRAY_TPS_TILE_SIDE 22            // 16 + 2 * 3
#define FRAY_TPS_TILE_TEXELS (FRAY_TPS_TILE_SIDE * FRAY_TPS_TILE_SIDE)

static __global__ __launch_bounds__(256) void k_tp_variance_split(TemporalSplitCall T)
{
    const int W = T.W, H = T.H;
    __shared__ float4 tile[3 * FRAY_TPS_TILE_TEXELS];
    float4* const tile1 = tile;                                 // {P.xyz, m1_D}
    float4* const tile2 = tile + FRAY_TPS_TILE_TEXELS;          // {n.xyz, m2_D}
    float4* const tile4 = tile + 2 * FRAY_TPS_TILE_TEXELS;      // {m1_I, m2_I, 0, 0}
    const int tilesX = (W + 15) / 16;                // the tiles in row-major order along grid x, as k_tp_variance's
    const int bx = (int)(blockIdx.x % (unsigned)tilesX) * 16, by = (int)(blockIdx.x / (unsigned)tilesX) * 16;
    const int lx = (int)threadIdx.x & 15, ly = (int)threadIdx.x >> 4;
    const int x = bx + lx, y = by + ly;
    const bool inside = x < W && y < H;
    const size_t p = inside ? (size_t)y * W + x : 0;
    const float4* hp = T.histOut + p * FRAY_TPS_ROWS;
    const float ND = hp[0].w, NI = hp[3].w;
    const bool youngD = inside && ND < (float)T.varianceHistory[0], youngI = inside && NI < (float)T.varianceHistory[1];
    if (!__syncthreads_or(youngD || youngI)) return;            // a block whose pixels all have both histories stages nothing
    for (int t = (int)threadIdx.x; t < FRAY_TPS_TILE_TEXELS; t += 256) {
        const int ty = t / FRAY_TPS_TILE_SIDE, tx = t - ty * FRAY_TPS_TILE_SIDE;
        const int xq = bx + tx - 3, yq = by + ty - 3;
        if (xq >= 0 && xq < W && yq >= 0 && yq < H) {
            const float4* hq = T.histOut + ((size_t)yq * W + xq) * FRAY_TPS_ROWS;
            tile1[t] = hq[1];
            tile2[t] = hq[2];
            tile4[t] = hq[4];
        }
    }
    __syncthreads();
    if (!(youngD || youngI)) return;
    const float4 p1 = hp[1], p2 = hp[2], p4 = hp[4];
    const bool pZero = p2.x == 0.0f && p2.y == 0.0f && p2.z == 0.0f;
    const float tol = T.planeTolerance * T.feat[p * FRAYHIP_FEAT_CHANNELS + 9];
    float s1d = 0.0f, s2d = 0.0f, s1i = 0.0f, s2i = 0.0f, cnt = 0.0f;
    for (int j = -3; j <= 3; j++) {
        const int yq = y + j;
        if (yq < 0 || yq >= H) continue;
        for (int i = -3; i <= 3; i++) {
            const int xq = x + i;
            if (xq < 0 || xq >= W) continue;
            const int t = (ly + 3 + j) * FRAY_TPS_TILE_SIDE + (lx + 3 + i);
            const float4 q1 = tile1[t], q2 = tile2[t];
            const bool qZero = q2.x == 0.0f && q2.y == 0.0f && q2.z == 0.0f;
            if (pZero || qZero) {
                if (!(pZero && qZero)) continue;
            } else {
                if (!(tp_dot(p2.x, p2.y, p2.z, q2.x, q2.y, q2.z) >= T.normalMinDot)) continue;
                if (!(fabsf(tp_dot(q1.x - p1.x, q1.y - p1.y, q1.z - p1.z, p2.x, p2.y, p2.z)) <= tol)) continue;
            }
            const float4 q4 = tile4[t];
            s1d += q1.w; s2d += q2.w;
            s1i += q4.x; s2i += q4.y;
            cnt += 1.0f;
        }
    }
    float mean1d = p1.w, mean2d = p2.w, mean1i = p4.x, mean2i = p4.y;
    if (cnt > 0.0f) { mean1d = s1d / cnt; mean2d = s2d / cnt; mean1i = s1i / cnt; mean2i = s2i / cnt; }
    if (youngD) T.variance[0][p] = fmaxf(0.0f, mean2d - mean1d * mean1d) * ((float)T.varianceHistory[0] / ND);
    if (youngI) T.variance[1][p] = fmaxf(0.0f, mean2i - mean1i * mean1i) * ((float)T.varianceHistory[1] / NI);
}

namespace {

using namespace frayhip_detail;
using namespace frayhip_temporal_detail;

struct SplitArgs {
    const float *rgbD, *rgbI, *feat, *motion, *histIn;
    const frayhip_view* view;
    const struct frayhip_temporal *pD, *pI;
    float *histOut, *signalD, *signalI, *varD, *varI;
    const float *chgD = nullptr, *chgI = nullptr;       // the _adaptive entries' change frames
};

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// Every check of the entries, in frayhip_temporal_accumulate's order; none touches the device.  adaptive: the _adaptive entries, whose change
// frames are inputs like feat.
int check(const char* who, int W, int H, const SplitArgs& A, bool device, bool adaptive = false)
{
    if (W < 1 || H < 1) return bad(who, "width and height must be >= 1");
    if ((long long)W * H > (1ll << 30)) return bad(who, "more than 2^30 pixels");
    if (!A.rgbD) return bad(who, "null rgb_direct");
    if (!A.rgbI) return bad(who, "null rgb_indirect");
    if (!A.feat) return bad(who, "null feat");
    if (adaptive && !A.chgD) return bad(who, "null change_direct");
    if (adaptive && !A.chgI) return bad(who, "null change_indirect");
    if (!A.pD) return bad(who, "null p_direct");
    if (!A.pI) return bad(who, "null p_indirect");
    if (!A.histOut) return bad(who, "null hist_out");
    if (!A.signalD) return bad(who, "null signal_direct");
    if (!A.signalI) return bad(who, "null signal_indirect");
    if (!A.varD) return bad(who, "null variance_direct");
    if (!A.varI) return bad(who, "null variance_indirect");
    if (!A.histIn != !A.view) return bad(who, "hist_in and prev_view must both be given or both be null");
    if (device) {
        for (const void* q : {(const void*)A.rgbD, (const void*)A.rgbI, (const void*)A.feat, (const void*)A.signalD, (const void*)A.signalI, (const void*)A.varD,
                              (const void*)A.varI, (const void*)A.chgD, (const void*)A.chgI})
            if (misaligned(q, 4)) return bad(who, "device pointer to floats not 4-byte aligned");
        if (misaligned(A.histIn, 16) || misaligned(A.histOut, 16)) return bad(who, "device pointer to a history not 16-byte aligned");
        if (misaligned(A.motion, 16)) return bad(who, "device pointer to a motion frame not 16-byte aligned");
    }
    if (const int rc = check_view(who, W, H, A.view)) return rc;
    if (const int rc = check_params(who, A.pD, "p_direct: ")) return rc;
    if (const int rc = check_params(who, A.pI, "p_indirect: ")) return rc;
    // the fields that decide which taps count, bit for bit
    if (A.pD->demodulate != A.pI->demodulate) return bad(who, "p_direct and p_indirect differ in demodulate");
    if (!same_bits(A.pD->film_offset, A.pI->film_offset)) return bad(who, "p_direct and p_indirect differ in film_offset");
    if (!same_bits(A.pD->plane_tolerance, A.pI->plane_tolerance)) return bad(who, "p_direct and p_indirect differ in plane_tolerance");
    if (!same_bits(A.pD->normal_min_dot, A.pI->normal_min_dot)) return bad(who, "p_direct and p_indirect differ in normal_min_dot");
    const size_t n = (size_t)W * H;
    const struct { const void* q; size_t bytes; } ins[7] = {{A.rgbD, 12 * n}, {A.rgbI, 12 * n}, {A.feat, 4 * FRAYHIP_FEAT_CHANNELS * n},
                                                            {A.histIn, 4 * FRAYHIP_HISTORY_SPLIT_CHANNELS * n}, {A.motion, 4 * FRAYHIP_MOTION_CHANNELS * n},
                                                            {A.chgD, 4 * n}, {A.chgI, 4 * n}};
    const struct { const void* q; size_t bytes; const char* name; } outs[5] = {{A.histOut, 4 * FRAYHIP_HISTORY_SPLIT_CHANNELS * n, "hist_out"},
                                                                                 {A.signalD, 12 * n, "signal_direct"}, {A.signalI, 12 * n, "signal_indirect"},
                                                                                 {A.varD, 4 * n, "variance_direct"}, {A.varI, 4 * n, "variance_indirect"}};
    for (int o = 0; o < 5; o++) {
        for (const auto& in : ins)
            if (overlaps(outs[o].q, outs[o].bytes, in.q, in.bytes)) return bad(who, std::string(outs[o].name) + " must not overlap an input");
        for (int k = 0; k < o; k++)
            if (overlaps(outs[o].q, outs[o].bytes, outs[k].q, outs[k].bytes)) return bad(who, std::string(outs[o].name) + " must not overlap " + outs[k].name);
    }
    return FRAYHIP_OK;
}

// The device path of the entries (device pointers, checked); with change frames the <MOTION, true> kernels
int run(int W, int H, const SplitArgs& A, hipStream_t stream, frayhip_stats* st, std::chrono::steady_clock::time_point t0)
{
    const size_t n = (size_t)W * H;
    TemporalSplitCall T{};
    T.W = W; T.H = H;
    T.rgb[0] = A.rgbD; T.rgb[1] = A.rgbI; T.feat = A.feat; T.motion = (const float4*)A.motion;
    T.histIn = (const float4*)A.histIn; T.histOut = (float4*)A.histOut;
    T.signal[0] = A.signalD; T.signal[1] = A.signalI; T.variance[0] = A.varD; T.variance[1] = A.varI;
    T.change[0] = A.chgD; T.change[1] = A.chgI;
    if (A.view) T.view = *A.view;
    T.demodulate = A.pD->demodulate;
    T.varianceHistory[0] = A.pD->variance_history; T.varianceHistory[1] = A.pI->variance_history;
    T.maxHistory[0] = (float)A.pD->max_history; T.maxHistory[1] = (float)A.pI->max_history;
    T.alphaMin[0] = A.pD->alpha_min; T.alphaMin[1] = A.pI->alpha_min;
    T.filmOffset = A.pD->film_offset; T.planeTolerance = A.pD->plane_tolerance; T.normalMinDot = A.pD->normal_min_dot;
    Events E;
    HIP_TRY(hipEventCreate(&E.a));
    HIP_TRY(hipEventCreate(&E.b));
    struct Drain { hipStream_t s; bool armed = true; ~Drain() { if (armed) (void)hipStreamSynchronize(s); } } drain{stream};
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    HIP_TRY(hipEventRecord(E.a, stream));
    if (A.chgD && A.motion) hipLaunchKernelGGL((k_tp_accumulate_split<true, true>), grid, block, 0, stream, T);
    else if (A.chgD) hipLaunchKernelGGL((k_tp_accumulate_split<false, true>), grid, block, 0, stream, T);
    else if (A.motion) hipLaunchKernelGGL((k_tp_accumulate_split<true, false>), grid, block, 0, stream, T);
    else hipLaunchKernelGGL((k_tp_accumulate_split<false, false>), grid, block, 0, stream, T);
    HIP_TRY(hipGetLastError());
    if (A.pD->variance_history > 1 || A.pI->variance_history > 1) {     // N >= 1 always: a component with variance_history 1 never takes the window
        hipLaunchKernelGGL(k_tp_variance_split, dim3((unsigned)((W + 15) / 16) * (unsigned)((H + 15) / 16)), block, 0, stream, T);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(E.b, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    if (st) {
        frayhip_stats o{};
        float ms = 0;
        (void)hipEventElapsedTime(&ms, E.a, E.b);
        o.ms_kernels = ms;
        o.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *st = o;
    }
    return FRAYHIP_OK;
}

// The host path of the entries (host pointers): checked, staged in one allocation, run on the null stream, copied back
int run_host(const char* who, int width, int height, const SplitArgs& A, bool adaptive, frayhip_stats* st, std::chrono::steady_clock::time_point t0)
{
    if (const int rc = check(who, width, height, A, false, adaptive)) return rc;
    const size_t n = (size_t)width * height;
    const size_t HC = FRAYHIP_HISTORY_SPLIT_CHANNELS, MC = FRAYHIP_MOTION_CHANNELS, FC = FRAYHIP_FEAT_CHANNELS;
    // one allocation, the 16-byte rows first: hist_out, hist_in and motion when given, then both rgb, feat, both change frames when given, both
    // signals, both variances
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_hout;
    if (const int rc = B.alloc(d_hout, n * (HC + (A.histIn ? HC : 0) + (A.motion ? MC : 0) + 6 + FC + (adaptive ? 2 : 0) + 6 + 2))) return rc;
    float* q = d_hout + HC * n;
    float* d_hin = nullptr;
    float* d_motion = nullptr;
    if (A.histIn) { d_hin = q; q += HC * n; }
    if (A.motion) { d_motion = q; q += MC * n; }
    float* d_rgbD = q;
    float* d_rgbI = d_rgbD + 3 * n;
    float* d_feat = d_rgbI + 3 * n;
    q = d_feat + FC * n;
    float* d_chgD = nullptr;
    float* d_chgI = nullptr;
    if (adaptive) { d_chgD = q; d_chgI = q + n; q += 2 * n; }
    float* d_sigD = q;
    float* d_sigI = d_sigD + 3 * n;
    float* d_varD = d_sigI + 3 * n;
    float* d_varI = d_varD + n;
    HIP_TRY(hipMemcpy(d_rgbD, A.rgbD, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_rgbI, A.rgbI, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_feat, A.feat, n * 4 * FC, hipMemcpyHostToDevice));
    if (adaptive) {
        HIP_TRY(hipMemcpy(d_chgD, A.chgD, n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_chgI, A.chgI, n * 4, hipMemcpyHostToDevice));
    }
    if (d_motion) HIP_TRY(hipMemcpy(d_motion, A.motion, n * 4 * MC, hipMemcpyHostToDevice));
    if (d_hin) HIP_TRY(hipMemcpy(d_hin, A.histIn, n * 4 * HC, hipMemcpyHostToDevice));
    const SplitArgs D{d_rgbD, d_rgbI, d_feat, d_motion, d_hin, A.view, A.pD, A.pI, d_hout, d_sigD, d_sigI, d_varD, d_varI, d_chgD, d_chgI};
    if (const int rc = run(width, height, D, nullptr, st, t0)) return rc;
    HIP_TRY(hipMemcpy(A.histOut, d_hout, n * 4 * HC, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(A.signalD, d_sigD, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(A.signalI, d_sigI, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(A.varD, d_varD, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(A.varI, d_varI, n * 4, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

}  // namespace

extern "C" {

int frayhip_temporal_accumulate_split_device(int width, int height, const float* d_rgb_direct, const float* d_rgb_indirect, const float* d_feat, const float* d_motion,
                                             const frayhip_view* prev_view, const float* d_hist_in, const struct frayhip_temporal* p_direct,
                                             const struct frayhip_temporal* p_indirect, float* d_hist_out, float* d_signal_direct, float* d_signal_indirect,
                                             float* d_variance_direct, float* d_variance_indirect, void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const SplitArgs A{d_rgb_direct, d_rgb_indirect, d_feat, d_motion, d_hist_in, prev_view, p_direct, p_indirect,
                      d_hist_out, d_signal_direct, d_signal_indirect, d_variance_direct, d_variance_indirect};
    if (const int rc = check("frayhip_temporal_accumulate_split_device", width, height, A, true)) return rc;
    return run(width, height, A, (hipStream_t)hip_stream, st, t0);
}

int frayhip_temporal_accumulate_split(int width, int height, const float* rgb_direct, const float* rgb_indirect, const float* feat, const float* motion,
                                      const frayhip_view* prev_view, const float* hist_in, const struct frayhip_temporal* p_direct,
                                      const struct frayhip_temporal* p_indirect, float* hist_out, float* signal_direct, float* signal_indirect,
                                      float* variance_direct, float* variance_indirect, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const SplitArgs A{rgb_direct, rgb_indirect, feat, motion, hist_in, prev_view, p_direct, p_indirect,
                      hist_out, signal_direct, signal_indirect, variance_direct, variance_indirect};
    return run_host("frayhip_temporal_accumulate_split", width, height, A, false, st, t0);
}

int frayhip_temporal_accumulate_split_adaptive_device(int width, int height, const float* d_rgb_direct, const float* d_rgb_indirect, const float* d_feat,
                                                      const float* d_motion, const float* d_change_direct, const float* d_change_indirect,
                                                      const frayhip_view* prev_view, const float* d_hist_in, const struct frayhip_temporal* p_direct,
                                                      const struct frayhip_temporal* p_indirect, float* d_hist_out, float* d_signal_direct,
                                                      float* d_signal_indirect, float* d_variance_direct, float* d_variance_indirect, void* hip_stream,
                                                      frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const SplitArgs A{d_rgb_direct, d_rgb_indirect, d_feat, d_motion, d_hist_in, prev_view, p_direct, p_indirect,
                      d_hist_out, d_signal_direct, d_signal_indirect, d_variance_direct, d_variance_indirect, d_change_direct, d_change_indirect};
    if (const int rc = check("frayhip_temporal_accumulate_split_adaptive_device", width, height, A, true, true)) return rc;
    return run(width, height, A, (hipStream_t)hip_stream, st, t0);
}

int frayhip_temporal_accumulate_split_adaptive(int width, int height, const float* rgb_direct, const float* rgb_indirect, const float* feat, const float* motion,
                                               const float* change_direct, const float* change_indirect, const frayhip_view* prev_view, const float* hist_in,
                                               const struct frayhip_temporal* p_direct, const struct frayhip_temporal* p_indirect, float* hist_out,
                                               float* signal_direct, float* signal_indirect, float* variance_direct, float* variance_indirect,
                                               frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const SplitArgs A{rgb_direct, rgb_indirect, feat, motion, hist_in, prev_view, p_direct, p_indirect,
                      hist_out, signal_direct, signal_indirect, variance_direct, variance_indirect, change_direct, change_indirect};
    return run_host("frayhip_temporal_accumulate_split_adaptive", width, height, A, true, st, t0);
}

}  // extern "C"
