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
