// What temporal.hip and temporal_split.hip share: the luminance and the dot product in the order include/frayhip.h writes them down, and the
// host checks of a view and of a parameter struct (the messages are the entries'; none touches the device).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "entry_support.hpp"

static __device__ __forceinline__ float tp_lum(float r, float g, float b) { return ((r + g) + b) / 3.0f; }
static __device__ __forceinline__ float tp_dot(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// Steps 1 and 2 of the accumulation as k_tp_accumulate (temporal.hip) and k_hm_held (history_map.hip) both run them: one text, so that the map's
// `held` is the history the accumulation will fetch.
// TpSurface: the pixel's position and unit normal (k_dn_prepare's scaling), what is carried into the previous view -- the same, or with a
// motion frame where they were (P', n' scaled as the normal is) -- and whether the pixel takes no history at all.
struct TpSurface {
    float Px, Py, Pz, nx, ny, nz;
    float Qx, Qy, Qz, mx, my, mz;
    bool miss;
};

template <bool MOTION>
static __device__ __forceinline__ TpSurface tp_surface(const float* f, const float4* motion, size_t p)
{
    TpSurface s;
    s.Px = f[0]; s.Py = f[1]; s.Pz = f[2];
    float nx = f[3], ny = f[4], nz = f[5];
    const float nn = nx * nx + ny * ny + nz * nz;
    if (nn > 0.0f) {                       // k_dn_prepare's unit normal
        const float sc = sqrtf(nn);
        nx = nx / sc; ny = ny / sc; nz = nz / sc;
    }
    s.nx = nx; s.ny = ny; s.nz = nz;
    s.miss = nx == 0.0f && ny == 0.0f && nz == 0.0f;
    s.Qx = s.Px; s.Qy = s.Py; s.Qz = s.Pz; s.mx = nx; s.my = ny; s.mz = nz;
    if constexpr (MOTION) {
        const float4 r0 = motion[2 * p], r1 = motion[2 * p + 1];
        s.Qx = r0.x; s.Qy = r0.y; s.Qz = r0.z;
        float mx = r1.x, my = r1.y, mz = r1.z;
        const float mm = mx * mx + my * my + mz * mz;
        if (mm > 0.0f) {
            const float sc = sqrtf(mm);
            mx = mx / sc; my = my / sc; mz = mz / sc;
        }
        s.mx = mx; s.my = my; s.mz = mz;
        s.miss = s.miss || (mx == 0.0f && my == 0.0f && mz == 0.0f);
    }
    return s;
}

// The bilinear fetch: the weighted sums over the counted taps, in tap order (j outer), undivided; sb is the sum of their weights, 0 when no
// history is fetched (no histIn, a miss, zc <= 0, the footprint off the image, no counted tap).  hu: the same sum over the units plane, <UNITS> only.
struct TpFetch {
    float sb, hr, hg, hb, hn, h1, h2, hu;
};

template <bool UNITS>
static __device__ __forceinline__ TpFetch tp_fetch(const TpSurface& s, int W, int H, const float4* histIn, const float* unitsIn, const frayhip_view& V,
                                                   float filmOffset, float planeTolerance, float normalMinDot)
{
    TpFetch t{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (!histIn || s.miss) return t;
    const float dx = s.Qx - V.pos[0], dy = s.Qy - V.pos[1], dz = s.Qz - V.pos[2];
    const float zc = tp_dot(dx, dy, dz, V.front[0], V.front[1], V.front[2]);
    if (!(zc > 0.0f)) return t;
    const float xc = tp_dot(dx, dy, dz, V.right[0], V.right[1], V.right[2]);
    const float yc = tp_dot(dx, dy, dz, V.up[0], V.up[1], V.up[2]);
    const float fx = ((xc / zc / V.tan_x + 1.0f) * 0.5f) * (float)W;
    const float fy = ((1.0f - yc / zc / V.tan_y) * 0.5f) * (float)H;
    const float u = fx - filmOffset, v = fy - filmOffset;
    const float x0f = floorf(u), y0f = floorf(v);
    // a footprint that touches the image (the comparisons are false for a NaN): only then do the floats fit an int
    if (!(x0f >= -1.0f && x0f <= (float)(W - 1) && y0f >= -1.0f && y0f <= (float)(H - 1))) return t;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float tx = u - x0f, ty = v - y0f;
    const float tol = planeTolerance * sqrtf(tp_dot(dx, dy, dz, dx, dy, dz));
    for (int j = 0; j < 2; j++) {
        const int yq = y0 + j;
        if (yq < 0 || yq >= H) continue;
        for (int i = 0; i < 2; i++) {
            const int xq = x0 + i;
            if (xq < 0 || xq >= W) continue;
            const size_t q = (size_t)yq * W + xq;
            const float4* hq = histIn + q * 3;
            const float4 q0 = hq[0], q1 = hq[1], q2 = hq[2];
            if (q2.x == 0.0f && q2.y == 0.0f && q2.z == 0.0f) continue;
            if (!(tp_dot(s.mx, s.my, s.mz, q2.x, q2.y, q2.z) >= normalMinDot)) continue;
            if (!(fabsf(tp_dot(q1.x - s.Qx, q1.y - s.Qy, q1.z - s.Qz, s.mx, s.my, s.mz)) <= tol)) continue;
            const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
            t.sb += b;
            t.hr += b * q0.x; t.hg += b * q0.y; t.hb += b * q0.z; t.hn += b * q0.w;
            t.h1 += b * q1.w; t.h2 += b * q2.w;
            if constexpr (UNITS) t.hu += b * unitsIn[q];
        }
    }
    return t;
}

namespace frayhip_temporal_detail {

using frayhip_detail::bad;

inline bool overlaps(const void* a, size_t an, const void* b, size_t bn)
{
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

inline bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

inline int check_view(const char* who, int W, int H, const frayhip_view* view)
{
    if (!view) return FRAYHIP_OK;
    if (view->width != W || view->height != H) return bad(who, "prev_view's size is not the frame's");
    if (!finite3(view->pos) || !finite3(view->right) || !finite3(view->up) || !finite3(view->front) || !std::isfinite(view->tan_x) || !std::isfinite(view->tan_y))
        return bad(who, "prev_view has a non-finite field");
    if (!(view->tan_x > 0) || !(view->tan_y > 0)) return bad(who, "prev_view's tan_x and tan_y must be > 0");
    return FRAYHIP_OK;
}

// what: a prefix of the message that says whose struct it is ("" for the entries that take one)
inline int check_params(const char* who, const struct frayhip_temporal* p, const char* what = "")
{
    const std::string w(what);
    if (p->demodulate != 0 && p->demodulate != 1) return bad(who, w + "demodulate must be 0 or 1");
    if (p->max_history < 1 || p->max_history > 4096) return bad(who, w + "max_history must be 1..4096");
    if (p->variance_history < 1 || p->variance_history > 4096) return bad(who, w + "variance_history must be 1..4096");
    if (!(p->alpha_min >= 0 && p->alpha_min <= 1)) return bad(who, w + "alpha_min must be 0..1");
    if (!std::isfinite(p->film_offset)) return bad(who, w + "film_offset must be finite");
    if (!std::isfinite(p->plane_tolerance) || p->plane_tolerance < 0) return bad(who, w + "plane_tolerance must be finite and >= 0");
    if (!(p->normal_min_dot >= -1 && p->normal_min_dot <= 1)) return bad(who, w + "normal_min_dot must be -1..1");
    return FRAYHIP_OK;
}

struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

}  // namespace frayhip_temporal_detail
