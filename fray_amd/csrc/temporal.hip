// C ABI, temporal accumulation (include/frayhip.h "temporal accumulation"): frayhip_view_from_camera, frayhip_temporal_defaults,
// frayhip_temporal_accumulate, frayhip_temporal_accumulate_motion, frayhip_temporal_accumulate_adaptive and their _device entries.  The temporal stage of SVGF: the previous frame's accumulated signal and
// luminance moments reprojected through the feature frame's world positions, surface tests on the four bilinear taps, the exponential blend,
// and the variance the a-trous levels take (frayhip_denoise_signal).  Scene-free, FP32 throughout; the Makefile builds this object as it builds
// denoise.o (-ffp-contract=off, correctly rounded divide and sqrt), so every product and sum below is rounded where it is written
// (tests/temporal_ref.py restates it in numpy, and the two agree bit for bit).
//
//   k_tp_accumulate  per pixel: the signal, the projection into the previous view, four taps of three float4 rows each, the blend; writes the
//                    three history rows, the signal, and the temporal variance where N >= variance_history.  <MOTION>: the point projected and
//                    the surface the taps are tested against are the motion frame's P' and n' (two float4 rows) instead of the feature frame's
//                    position and normal; <false> is the kernel as it was.  <MOTION, ADAPTIVE>: a change frame (change.hip) shortens the history per
//                    pixel -- none where change >= 1, a blend factor raised towards 1 where it is > 0, the arithmetic as it was where it is 0;
//                    <MOTION, false> are the two kernels as they were.  <MOTION, ADAPTIVE, WEIGHTED> (frayhip_temporal_accumulate_weighted): the
//                    frame weighs w units and the history the hu units fetched from a units plane beside it, so the blend factor is w / U with
//                    U = min(hu + w, max_history) where the unweighted kernels have 1 / N; N, which k_tp_variance reads, still counts frames.
//                    With w = 1 and a units plane equal to the history's N channel bit for bit, hu is hn (the same products summed in the same
//                    order), so U is N and w / U is 1.0f / N on the same operands: every output bit is the <MOTION, ADAPTIVE, false> kernel's
//                    and units_out is hist_out's N.  <.., .., false> compiles the arithmetic as it was: every WEIGHTED branch is if constexpr
//                    Steps 1 and 2 (tp_surface, tp_fetch) are temporal_common.hpp's, shared with k_hm_held (history_map.hip)
//   k_tp_variance   per pixel with N < variance_history: the 7x7 window of the finished history (rows 1 and 2: position, normal, m1, m2),
//                    taken from an LDS tile that the 16x16 block stages first; a block without such a pixel stages nothing
// k_tp_accumulate's taps are read through L1 / L2, as the filter's.  k_tp_variance with the same direct reads took 0.214 ms at 1080p where
// every pixel takes the window, against 0.074 ms from the tile ("Temporal accumulation").
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>

#include "entry_support.hpp"
#include "temporal_common.hpp"

struct TemporalCall {
    int W, H;
    const float* rgb;
    const float* feat;
    const float4* motion;       // k_tp_accumulate<true> only: two rows a pixel
    const float4* histIn;       // null: first frame
    float4* histOut;
    float* signal;
    float* variance;
    frayhip_view view;          // read only with histIn
    int demodulate, varianceHistory;
    float maxHistory, alphaMin, filmOffset, planeTolerance, normalMinDot;
    const float* change;        // k_tp_accumulate<MOTION, true> only: one float a pixel
    const float* weight;        // k_tp_accumulate<MOTION, ADAPTIVE, true> only: the frame's sample weight, one float a pixel
    const float* unitsIn;       // and the units plane beside histIn (null with it)
    float* unitsOut;            // and the one beside histOut
};

template <bool MOTION, bool ADAPTIVE, bool WEIGHTED = false>
static __global__ __launch_bounds__(256) void k_tp_accumulate(TemporalCall T)
{
    const int W = T.W, H = T.H;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const float* f = T.feat + p * FRAYHIP_FEAT_CHANNELS;
    const TpSurface S = tp_surface<MOTION>(f, T.motion, p);
    const float* c = T.rgb + 3 * p;
    float cr = c[0], cg = c[1], cb = c[2];
    if (T.demodulate) { cr = cr / fmaxf(f[6], 1e-3f); cg = cg / fmaxf(f[7], 1e-3f); cb = cb / fmaxf(f[8], 1e-3f); }
    const float l = tp_lum(cr, cg, cb);
    const float l2 = l * l;

    const TpFetch h = tp_fetch<WEIGHTED>(S, W, H, T.histIn, T.unitsIn, T.view, T.filmOffset, T.planeTolerance, T.normalMinDot);
    const float sb = h.sb;
    float hr = h.hr, hg = h.hg, hb = h.hb, hn = h.hn, h1 = h.h1, h2 = h.h2, hu = h.hu;
    float w = 1.0f;                        // the frame's sample weight in this pixel: NaN, 0 and negatives count as 1
    if constexpr (WEIGHTED) {
        w = T.weight[p];
        if (!(w >= 1.0f)) w = 1.0f;
        w = fminf(w, T.maxHistory);
    }
    float ar = cr, ag = cg, ab = cb, m1 = l, m2 = l2, N = 1.0f, U = w;
    float g = 0.0f;                        // the pixel's change, read only where a history was fetched
    if constexpr (ADAPTIVE) {
        if (sb > 0.0f) g = T.change[p];
    }
    if (ADAPTIVE && !(g < 1.0f)) {
        // changed through and through (1, above 1, NaN): no history, the first-frame values above
    } else if (ADAPTIVE && g > 0.0f) {
        hr = hr / sb; hg = hg / sb; hb = hb / sb; hn = hn / sb; h1 = h1 / sb; h2 = h2 / sb;
        const float N0 = fminf(hn + 1.0f, T.maxHistory);
        float a0, U0 = 0.0f;
        if constexpr (WEIGHTED) {
            hu = hu / sb;
            U0 = fminf(hu + w, T.maxHistory);
            a0 = fmaxf(T.alphaMin, w / U0);
        } else {
            a0 = fmaxf(T.alphaMin, 1.0f / N0);
        }
        const float alpha = a0 + g * (1.0f - a0);
        N = fminf(N0, 1.0f / alpha);
        if constexpr (WEIGHTED) U = fminf(U0, w / alpha);
        ar = hr + alpha * (cr - hr); ag = hg + alpha * (cg - hg); ab = hb + alpha * (cb - hb);
        m1 = h1 + alpha * (l - h1);
        m2 = h2 + alpha * (l2 - h2);
    } else if (sb > 0.0f) {
        hr = hr / sb; hg = hg / sb; hb = hb / sb; hn = hn / sb; h1 = h1 / sb; h2 = h2 / sb;
        N = fminf(hn + 1.0f, T.maxHistory);
        float alpha;
        if constexpr (WEIGHTED) {
            hu = hu / sb;
            U = fminf(hu + w, T.maxHistory);
            alpha = fmaxf(T.alphaMin, w / U);
        } else {
            alpha = fmaxf(T.alphaMin, 1.0f / N);
        }
        ar = hr + alpha * (cr - hr); ag = hg + alpha * (cg - hg); ab = hb + alpha * (cb - hb);
        m1 = h1 + alpha * (l - h1);
        m2 = h2 + alpha * (l2 - h2);
    }
    float4* ho = T.histOut + p * 3;
    ho[0] = make_float4(ar, ag, ab, N);
    ho[1] = make_float4(S.Px, S.Py, S.Pz, m1);
    ho[2] = make_float4(S.nx, S.ny, S.nz, m2);
    float* s = T.signal + 3 * p;
    s[0] = ar; s[1] = ag; s[2] = ab;
    if constexpr (WEIGHTED) T.unitsOut[p] = U;
    if (N >= (float)T.varianceHistory) T.variance[p] = fmaxf(0.0f, m2 - m1 * m1);
}

// A 16x16 block and the 22x22 texels its 7x7 windows reach: rows 1 and 2 of the history, 32 bytes a texel, 15.5 KB of LDS
#define FRAY_TP_TILE_SIDE 22            // 16 + 2 * 3

static __global__ __launch_bounds__(256) void k_tp_variance(TemporalCall T)
{
    const int W = T.W, H = T.H;
    __shared__ float4 tile[FRAY_TP_TILE_SIDE * FRAY_TP_TILE_SIDE * 2];
    const int tilesX = (W + 15) / 16;                // the tiles in row-major order along grid x (grid y would cap a tall image at 2^20 rows)
    const int bx = (int)(blockIdx.x % (unsigned)tilesX) * 16, by = (int)(blockIdx.x / (unsigned)tilesX) * 16;
    const int lx = (int)threadIdx.x & 15, ly = (int)threadIdx.x >> 4;
    const int x = bx + lx, y = by + ly;
    const bool inside = x < W && y < H;
    const size_t p = inside ? (size_t)y * W + x : 0;
    const float4* hp = T.histOut + p * 3;
    const float N = hp[0].w;
    const bool young = inside && N < (float)T.varianceHistory;
    if (!__syncthreads_or(young)) return;            // a block whose pixels all have their history stages nothing
    for (int t = (int)threadIdx.x; t < FRAY_TP_TILE_SIDE * FRAY_TP_TILE_SIDE; t += 256) {
        const int ty = t / FRAY_TP_TILE_SIDE, tx = t - ty * FRAY_TP_TILE_SIDE;
        const int xq = bx + tx - 3, yq = by + ty - 3;
        if (xq >= 0 && xq < W && yq >= 0 && yq < H) {
            const float4* hq = T.histOut + ((size_t)yq * W + xq) * 3;
            tile[2 * t] = hq[1];
            tile[2 * t + 1] = hq[2];
        }
    }
    __syncthreads();
    if (!young) return;
    const float4 p1 = hp[1], p2 = hp[2];
    const bool pZero = p2.x == 0.0f && p2.y == 0.0f && p2.z == 0.0f;
    const float tol = T.planeTolerance * T.feat[p * FRAYHIP_FEAT_CHANNELS + 9];
    float s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
    for (int j = -3; j <= 3; j++) {
        const int yq = y + j;
        if (yq < 0 || yq >= H) continue;
        for (int i = -3; i <= 3; i++) {
            const int xq = x + i;
            if (xq < 0 || xq >= W) continue;
            const int t = (ly + 3 + j) * FRAY_TP_TILE_SIDE + (lx + 3 + i);
            const float4 q1 = tile[2 * t], q2 = tile[2 * t + 1];
            const bool qZero = q2.x == 0.0f && q2.y == 0.0f && q2.z == 0.0f;
            if (pZero || qZero) {
                if (!(pZero && qZero)) continue;
            } else {
                if (!(tp_dot(p2.x, p2.y, p2.z, q2.x, q2.y, q2.z) >= T.normalMinDot)) continue;
                if (!(fabsf(tp_dot(q1.x - p1.x, q1.y - p1.y, q1.z - p1.z, p2.x, p2.y, p2.z)) <= tol)) continue;
            }
            s1 += q1.w; s2 += q2.w; cnt += 1.0f;
        }
    }
    float mean1 = p1.w, mean2 = p2.w;
    if (cnt > 0.0f) { mean1 = s1 / cnt; mean2 = s2 / cnt; }
    T.variance[p] = fmaxf(0.0f, mean2 - mean1 * mean1) * ((float)T.varianceHistory / N);
}

namespace {

using namespace frayhip_detail;
using namespace frayhip_temporal_detail;

// Every check of the entries, in this order; none touches the device.
// WITH_MOTION: the _motion entries, whose motion frame is an input like feat; NO_MOTION: the others (motion is null); MAY_MOTION: the _adaptive
// entries, which take either.  adaptive: the _adaptive entries, whose change frame is an input like feat.
enum MotionInput { NO_MOTION, WITH_MOTION, MAY_MOTION };
int check(const char* who, int W, int H, const float* rgb, const float* feat, const frayhip_view* view, const float* histIn, const struct frayhip_temporal* p,
          const float* histOut, const float* signal, const float* variance, bool device, MotionInput mi, const float* motion, bool adaptive = false,
          const float* change = nullptr)
{
    if (W < 1 || H < 1) return bad(who, "width and height must be >= 1");
    if ((long long)W * H > (1ll << 30)) return bad(who, "more than 2^30 pixels");
    if (!rgb) return bad(who, "null rgb");
    if (!feat) return bad(who, "null feat");
    if (mi == WITH_MOTION && !motion) return bad(who, "null motion");
    if (adaptive && !change) return bad(who, "null change");
    if (!p) return bad(who, "null parameters");
    if (!histOut) return bad(who, "null hist_out");
    if (!signal) return bad(who, "null signal");
    if (!variance) return bad(who, "null variance");
    if (!histIn != !view) return bad(who, "hist_in and prev_view must both be given or both be null");
    if (device) {
        for (const void* q : {(const void*)rgb, (const void*)feat, (const void*)signal, (const void*)variance, (const void*)change})
            if (misaligned(q, 4)) return bad(who, "device pointer to floats not 4-byte aligned");
        if (misaligned(histIn, 16) || misaligned(histOut, 16)) return bad(who, "device pointer to a history not 16-byte aligned");
        if (misaligned(motion, 16)) return bad(who, "device pointer to a motion frame not 16-byte aligned");
    }
    if (const int rc = check_view(who, W, H, view)) return rc;
    if (const int rc = check_params(who, p)) return rc;
    const size_t n = (size_t)W * H;
    const struct { const void* q; size_t bytes; } ins[5] = {{rgb, 12 * n}, {feat, 4 * FRAYHIP_FEAT_CHANNELS * n}, {histIn, 4 * FRAYHIP_HISTORY_CHANNELS * n},
                                                            {motion, 4 * FRAYHIP_MOTION_CHANNELS * n}, {change, 4 * n}};
    const struct { const void* q; size_t bytes; const char* name; } outs[3] = {{histOut, 4 * FRAYHIP_HISTORY_CHANNELS * n, "hist_out"}, {signal, 12 * n, "signal"},
                                                                                 {variance, 4 * n, "variance"}};
    for (int o = 0; o < 3; o++) {
        for (const auto& in : ins)
            if (overlaps(outs[o].q, outs[o].bytes, in.q, in.bytes)) return bad(who, std::string(outs[o].name) + " must not overlap an input");
        for (int k = 0; k < o; k++)
            if (overlaps(outs[o].q, outs[o].bytes, outs[k].q, outs[k].bytes)) return bad(who, std::string(outs[o].name) + " must not overlap " + outs[k].name);
    }
    return FRAYHIP_OK;
}

// The device path of the entries (device pointers, checked)
// motion: the motion frame of the _motion and _adaptive entries, or null; change: the change frame of the _adaptive entries, or null
int run(int W, int H, const float* rgb, const float* feat, const frayhip_view* view, const float* histIn, const struct frayhip_temporal* prm, float* histOut,
        float* signal, float* variance, hipStream_t stream, frayhip_stats* st, std::chrono::steady_clock::time_point t0, const float* motion = nullptr,
        const float* change = nullptr, const float* weight = nullptr, const float* unitsIn = nullptr, float* unitsOut = nullptr)
{
    const size_t n = (size_t)W * H;
    TemporalCall T{};
    T.W = W; T.H = H;
    T.rgb = rgb; T.feat = feat; T.motion = (const float4*)motion;
    T.histIn = (const float4*)histIn; T.histOut = (float4*)histOut;
    T.signal = signal; T.variance = variance; T.change = change;
    T.weight = weight; T.unitsIn = unitsIn; T.unitsOut = unitsOut;
    if (view) T.view = *view;
    T.demodulate = prm->demodulate; T.varianceHistory = prm->variance_history;
    T.maxHistory = (float)prm->max_history; T.alphaMin = prm->alpha_min; T.filmOffset = prm->film_offset;
    T.planeTolerance = prm->plane_tolerance; T.normalMinDot = prm->normal_min_dot;
    Events E;
    HIP_TRY(hipEventCreate(&E.a));
    HIP_TRY(hipEventCreate(&E.b));
    struct Drain { hipStream_t s; bool armed = true; ~Drain() { if (armed) (void)hipStreamSynchronize(s); } } drain{stream};
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    HIP_TRY(hipEventRecord(E.a, stream));
    if (weight && change && motion) hipLaunchKernelGGL((k_tp_accumulate<true, true, true>), grid, block, 0, stream, T);
    else if (weight && change) hipLaunchKernelGGL((k_tp_accumulate<false, true, true>), grid, block, 0, stream, T);
    else if (weight && motion) hipLaunchKernelGGL((k_tp_accumulate<true, false, true>), grid, block, 0, stream, T);
    else if (weight) hipLaunchKernelGGL((k_tp_accumulate<false, false, true>), grid, block, 0, stream, T);
    else if (change && motion) hipLaunchKernelGGL((k_tp_accumulate<true, true>), grid, block, 0, stream, T);
    else if (change) hipLaunchKernelGGL((k_tp_accumulate<false, true>), grid, block, 0, stream, T);
    else if (motion) hipLaunchKernelGGL((k_tp_accumulate<true, false>), grid, block, 0, stream, T);
    else hipLaunchKernelGGL((k_tp_accumulate<false, false>), grid, block, 0, stream, T);
    HIP_TRY(hipGetLastError());
    if (prm->variance_history > 1) {         // N >= 1 always: with variance_history 1 no pixel takes the spatial estimate
        hipLaunchKernelGGL(k_tp_variance, dim3((unsigned)((W + 15) / 16) * (unsigned)((H + 15) / 16)), block, 0, stream, T);
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

// The weighted entries' checks: the adaptive entry's list with motion and change both optional, then the weight plane and the two units planes
int check_weighted(const char* who, int W, int H, const float* rgb, const float* feat, const float* motion, const float* change, const float* weight,
                   const frayhip_view* view, const float* histIn, const float* unitsIn, const struct frayhip_temporal* p, const float* histOut,
                   const float* unitsOut, const float* signal, const float* variance, bool device)
{
    if (const int rc = check(who, W, H, rgb, feat, view, histIn, p, histOut, signal, variance, device, MAY_MOTION, motion, false, change)) return rc;
    if (!weight) return bad(who, "null weight");
    if (!unitsOut) return bad(who, "null units_out");
    if (!histIn != !unitsIn) return bad(who, "hist_in and units_in must both be given or both be null");
    if (device) {
        for (const void* q : {(const void*)weight, (const void*)unitsIn, (const void*)unitsOut})
            if (misaligned(q, 4)) return bad(who, "device pointer to floats not 4-byte aligned");
    }
    const size_t n = (size_t)W * H;
    const struct { const void* q; size_t bytes; const char* name; } ins[7] = {{rgb, 12 * n, "rgb"}, {feat, 4 * FRAYHIP_FEAT_CHANNELS * n, "feat"},
                                                                              {histIn, 4 * FRAYHIP_HISTORY_CHANNELS * n, "hist_in"},
                                                                              {motion, 4 * FRAYHIP_MOTION_CHANNELS * n, "motion"}, {change, 4 * n, "change"},
                                                                              {weight, 4 * n, "weight"}, {unitsIn, 4 * n, "units_in"}};
    const struct { const void* q; size_t bytes; const char* name; } outs[3] = {{histOut, 4 * FRAYHIP_HISTORY_CHANNELS * n, "hist_out"}, {signal, 12 * n, "signal"},
                                                                                 {variance, 4 * n, "variance"}};
    for (const auto& o : outs) {
        for (int k = 5; k < 7; k++)
            if (overlaps(o.q, o.bytes, ins[k].q, ins[k].bytes)) return bad(who, std::string(o.name) + " must not overlap " + ins[k].name);
        if (overlaps(unitsOut, 4 * n, o.q, o.bytes)) return bad(who, std::string("units_out must not overlap ") + o.name);
    }
    for (const auto& in : ins)
        if (overlaps(unitsOut, 4 * n, in.q, in.bytes)) return bad(who, "units_out must not overlap an input");
    return FRAYHIP_OK;
}

}  // namespace

extern "C" {

int frayhip_view_from_camera(const frayhip_camera* c, int width, int height, frayhip_view* out)
{
    const char* who = "frayhip_view_from_camera";
    if (!c) return bad(who, "null camera");
    if (!out) return bad(who, "null view");
    if (width < 1 || height < 1) return bad(who, "width and height must be >= 1");
    for (const double v : {c->pos[0], c->pos[1], c->pos[2], c->yaw, c->pitch, c->roll, c->fov, c->aspectRatio})
        if (!std::isfinite(v)) return bad(who, "pos, yaw, pitch, roll, fov and aspectRatio must be finite");
    if (!(c->fov > 0 && c->fov < 180)) return bad(who, "fov must be inside (0, 180)");
    if (!(c->aspectRatio > 0)) return bad(who, "aspectRatio must be > 0");
    const DCamera f = camera_begin_frame(*c, width, height);
    // m of Camera::beginFrame, as camera_begin_frame derives it: the corners are rotations of (+-aspect * m, +-m, 1)
    const double PI = 3.141592653589793238;
    const double aspect = c->aspectRatio;
    const double m = tan(c->fov / 2 / 180.0 * PI) / sqrt(aspect * aspect + 1.0);
    frayhip_view v{};
    for (int k = 0; k < 3; k++) {
        v.pos[k] = (float)f.pos[k];
        v.right[k] = (float)f.rightDir[k];
        v.up[k] = (float)f.upDir[k];
        v.front[k] = (float)f.frontDir[k];
    }
    v.tan_x = (float)(aspect * m);
    v.tan_y = (float)m;
    v.width = width; v.height = height;
    if (!finite3(v.pos) || !(v.tan_x > 0) || !(v.tan_y > 0) || !std::isfinite(v.tan_x) || !std::isfinite(v.tan_y))
        return bad(who, "the camera does not round to a finite FP32 view");
    *out = v;
    return FRAYHIP_OK;
}

int frayhip_temporal_defaults(struct frayhip_temporal* p)
{
    if (!p) return bad("frayhip_temporal_defaults", "null parameters");
    p->demodulate = 1;
    p->max_history = 32;
    p->variance_history = 4;
    p->alpha_min = 0.05f;
    p->film_offset = 0.5f;
    p->plane_tolerance = 0.02f;
    p->normal_min_dot = 0.9f;
    return FRAYHIP_OK;
}

int frayhip_temporal_accumulate_device(int width, int height, const float* d_rgb, const float* d_feat, const frayhip_view* prev_view, const float* d_hist_in,
                                       const struct frayhip_temporal* p, float* d_hist_out, float* d_signal, float* d_variance, void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = check("frayhip_temporal_accumulate_device", width, height, d_rgb, d_feat, prev_view, d_hist_in, p, d_hist_out, d_signal, d_variance, true, NO_MOTION, nullptr))
        return rc;
    return run(width, height, d_rgb, d_feat, prev_view, d_hist_in, p, d_hist_out, d_signal, d_variance, (hipStream_t)hip_stream, st, t0);
}

int frayhip_temporal_accumulate(int width, int height, const float* rgb, const float* feat, const frayhip_view* prev_view, const float* hist_in,
                                const struct frayhip_temporal* p, float* hist_out, float* signal, float* variance, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_temporal_accumulate";
    if (const int rc = check(who, width, height, rgb, feat, prev_view, hist_in, p, hist_out, signal, variance, false, NO_MOTION, nullptr)) return rc;
    const size_t n = (size_t)width * height;
    const size_t HC = FRAYHIP_HISTORY_CHANNELS;
    // one allocation, the histories first (16-byte rows): hist_out, hist_in when given, then rgb, feat, signal, variance
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_hout;
    if (const int rc = B.alloc(d_hout, n * (HC + (hist_in ? HC : 0) + 3 + FRAYHIP_FEAT_CHANNELS + 3 + 1))) return rc;
    float* d_hin = hist_in ? d_hout + HC * n : nullptr;
    float* d_rgb = d_hout + HC * n * (hist_in ? 2 : 1);
    float* d_feat = d_rgb + 3 * n;
    float* d_signal = d_feat + FRAYHIP_FEAT_CHANNELS * n;
    float* d_var = d_signal + 3 * n;
    HIP_TRY(hipMemcpy(d_rgb, rgb, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_feat, feat, n * 4 * FRAYHIP_FEAT_CHANNELS, hipMemcpyHostToDevice));
    if (d_hin) HIP_TRY(hipMemcpy(d_hin, hist_in, n * 4 * HC, hipMemcpyHostToDevice));
    if (const int rc = run(width, height, d_rgb, d_feat, prev_view, d_hin, p, d_hout, d_signal, d_var, nullptr, st, t0)) return rc;
    HIP_TRY(hipMemcpy(hist_out, d_hout, n * 4 * HC, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(signal, d_signal, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(variance, d_var, n * 4, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

int frayhip_temporal_accumulate_motion_device(int width, int height, const float* d_rgb, const float* d_feat, const float* d_motion, const frayhip_view* prev_view,
                                              const float* d_hist_in, const struct frayhip_temporal* p, float* d_hist_out, float* d_signal, float* d_variance,
                                              void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = check("frayhip_temporal_accumulate_motion_device", width, height, d_rgb, d_feat, prev_view, d_hist_in, p, d_hist_out, d_signal, d_variance, true,
                             WITH_MOTION, d_motion))
        return rc;
    return run(width, height, d_rgb, d_feat, prev_view, d_hist_in, p, d_hist_out, d_signal, d_variance, (hipStream_t)hip_stream, st, t0, d_motion);
}

int frayhip_temporal_accumulate_motion(int width, int height, const float* rgb, const float* feat, const float* motion, const frayhip_view* prev_view,
                                       const float* hist_in, const struct frayhip_temporal* p, float* hist_out, float* signal, float* variance, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_temporal_accumulate_motion";
    if (const int rc = check(who, width, height, rgb, feat, prev_view, hist_in, p, hist_out, signal, variance, false, WITH_MOTION, motion)) return rc;
    const size_t n = (size_t)width * height;
    const size_t HC = FRAYHIP_HISTORY_CHANNELS, MC = FRAYHIP_MOTION_CHANNELS;
    // one allocation, the 16-byte rows first: hist_out, hist_in when given, motion, then rgb, feat, signal, variance
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_hout;
    if (const int rc = B.alloc(d_hout, n * (HC + (hist_in ? HC : 0) + MC + 3 + FRAYHIP_FEAT_CHANNELS + 3 + 1))) return rc;
    float* d_hin = hist_in ? d_hout + HC * n : nullptr;
    float* d_motion = d_hout + HC * n * (hist_in ? 2 : 1);
    float* d_rgb = d_motion + MC * n;
    float* d_feat = d_rgb + 3 * n;
    float* d_signal = d_feat + FRAYHIP_FEAT_CHANNELS * n;
    float* d_var = d_signal + 3 * n;
    HIP_TRY(hipMemcpy(d_rgb, rgb, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_feat, feat, n * 4 * FRAYHIP_FEAT_CHANNELS, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_motion, motion, n * 4 * MC, hipMemcpyHostToDevice));
    if (d_hin) HIP_TRY(hipMemcpy(d_hin, hist_in, n * 4 * HC, hipMemcpyHostToDevice));
    if (const int rc = run(width, height, d_rgb, d_feat, prev_view, d_hin, p, d_hout, d_signal, d_var, nullptr, st, t0, d_motion)) return rc;
    HIP_TRY(hipMemcpy(hist_out, d_hout, n * 4 * HC, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(signal, d_signal, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(variance, d_var, n * 4, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

int frayhip_temporal_accumulate_adaptive_device(int width, int height, const float* d_rgb, const float* d_feat, const float* d_motion, const float* d_change,
                                                const frayhip_view* prev_view, const float* d_hist_in, const struct frayhip_temporal* p, float* d_hist_out,
                                                float* d_signal, float* d_variance, void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = check("frayhip_temporal_accumulate_adaptive_device", width, height, d_rgb, d_feat, prev_view, d_hist_in, p, d_hist_out, d_signal, d_variance,
                             true, MAY_MOTION, d_motion, true, d_change))
        return rc;
    return run(width, height, d_rgb, d_feat, prev_view, d_hist_in, p, d_hist_out, d_signal, d_variance, (hipStream_t)hip_stream, st, t0, d_motion, d_change);
}

int frayhip_temporal_accumulate_adaptive(int width, int height, const float* rgb, const float* feat, const float* motion, const float* change,
                                         const frayhip_view* prev_view, const float* hist_in, const struct frayhip_temporal* p, float* hist_out, float* signal,
                                         float* variance, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_temporal_accumulate_adaptive";
    if (const int rc = check(who, width, height, rgb, feat, prev_view, hist_in, p, hist_out, signal, variance, false, MAY_MOTION, motion, true, change)) return rc;
    const size_t n = (size_t)width * height;
    const size_t HC = FRAYHIP_HISTORY_CHANNELS, MC = FRAYHIP_MOTION_CHANNELS;
    // one allocation, the 16-byte rows first: hist_out, hist_in and motion when given, then rgb, feat, change, signal, variance
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_hout;
    if (const int rc = B.alloc(d_hout, n * (HC + (hist_in ? HC : 0) + (motion ? MC : 0) + 3 + FRAYHIP_FEAT_CHANNELS + 1 + 3 + 1))) return rc;
    float* q = d_hout + HC * n;
    float* d_hin = nullptr;
    float* d_motion = nullptr;
    if (hist_in) { d_hin = q; q += HC * n; }
    if (motion) { d_motion = q; q += MC * n; }
    float* d_rgb = q;
    float* d_feat = d_rgb + 3 * n;
    float* d_change = d_feat + FRAYHIP_FEAT_CHANNELS * n;
    float* d_signal = d_change + n;
    float* d_var = d_signal + 3 * n;
    HIP_TRY(hipMemcpy(d_rgb, rgb, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_feat, feat, n * 4 * FRAYHIP_FEAT_CHANNELS, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_change, change, n * 4, hipMemcpyHostToDevice));
    if (d_motion) HIP_TRY(hipMemcpy(d_motion, motion, n * 4 * MC, hipMemcpyHostToDevice));
    if (d_hin) HIP_TRY(hipMemcpy(d_hin, hist_in, n * 4 * HC, hipMemcpyHostToDevice));
    if (const int rc = run(width, height, d_rgb, d_feat, prev_view, d_hin, p, d_hout, d_signal, d_var, nullptr, st, t0, d_motion, d_change)) return rc;
    HIP_TRY(hipMemcpy(hist_out, d_hout, n * 4 * HC, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(signal, d_signal, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(variance, d_var, n * 4, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

int frayhip_temporal_accumulate_weighted_device(int width, int height, const float* d_rgb, const float* d_feat, const float* d_motion, const float* d_change,
                                                const float* d_weight, const frayhip_view* prev_view, const float* d_hist_in, const float* d_units_in,
                                                const struct frayhip_temporal* p, float* d_hist_out, float* d_units_out, float* d_signal, float* d_variance,
                                                void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = check_weighted("frayhip_temporal_accumulate_weighted_device", width, height, d_rgb, d_feat, d_motion, d_change, d_weight, prev_view, d_hist_in,
                                      d_units_in, p, d_hist_out, d_units_out, d_signal, d_variance, true))
        return rc;
    return run(width, height, d_rgb, d_feat, prev_view, d_hist_in, p, d_hist_out, d_signal, d_variance, (hipStream_t)hip_stream, st, t0, d_motion, d_change, d_weight,
               d_units_in, d_units_out);
}

int frayhip_temporal_accumulate_weighted(int width, int height, const float* rgb, const float* feat, const float* motion, const float* change, const float* weight,
                                         const frayhip_view* prev_view, const float* hist_in, const float* units_in, const struct frayhip_temporal* p,
                                         float* hist_out, float* units_out, float* signal, float* variance, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_temporal_accumulate_weighted";
    if (const int rc = check_weighted(who, width, height, rgb, feat, motion, change, weight, prev_view, hist_in, units_in, p, hist_out, units_out, signal, variance, false))
        return rc;
    const size_t n = (size_t)width * height;
    const size_t HC = FRAYHIP_HISTORY_CHANNELS, MC = FRAYHIP_MOTION_CHANNELS;
    // one allocation, the 16-byte rows first: hist_out, hist_in and motion when given, then rgb, feat, weight, units_out, signal, variance, and
    // change and units_in when given
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_hout;
    if (const int rc = B.alloc(d_hout, n * (HC + (hist_in ? HC + 1 : 0) + (motion ? MC : 0) + 3 + FRAYHIP_FEAT_CHANNELS + 1 + 1 + 3 + 1 + (change ? 1 : 0)))) return rc;
    float* q = d_hout + HC * n;
    float* d_hin = nullptr;
    float* d_motion = nullptr;
    float* d_change = nullptr;
    float* d_uin = nullptr;
    if (hist_in) { d_hin = q; q += HC * n; }
    if (motion) { d_motion = q; q += MC * n; }
    float* d_rgb = q;
    float* d_feat = d_rgb + 3 * n;
    float* d_weight = d_feat + FRAYHIP_FEAT_CHANNELS * n;
    float* d_uout = d_weight + n;
    float* d_signal = d_uout + n;
    float* d_var = d_signal + 3 * n;
    q = d_var + n;
    if (change) { d_change = q; q += n; }
    if (hist_in) { d_uin = q; q += n; }
    HIP_TRY(hipMemcpy(d_rgb, rgb, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_feat, feat, n * 4 * FRAYHIP_FEAT_CHANNELS, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_weight, weight, n * 4, hipMemcpyHostToDevice));
    if (d_change) HIP_TRY(hipMemcpy(d_change, change, n * 4, hipMemcpyHostToDevice));
    if (d_motion) HIP_TRY(hipMemcpy(d_motion, motion, n * 4 * MC, hipMemcpyHostToDevice));
    if (d_hin) HIP_TRY(hipMemcpy(d_hin, hist_in, n * 4 * HC, hipMemcpyHostToDevice));
    if (d_uin) HIP_TRY(hipMemcpy(d_uin, units_in, n * 4, hipMemcpyHostToDevice));
    if (const int rc = run(width, height, d_rgb, d_feat, prev_view, d_hin, p, d_hout, d_signal, d_var, nullptr, st, t0, d_motion, d_change, d_weight, d_uin, d_uout))
        return rc;
    HIP_TRY(hipMemcpy(hist_out, d_hout, n * 4 * HC, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(units_out, d_uout, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(signal, d_signal, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(variance, d_var, n * 4, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

}  // extern "C"
