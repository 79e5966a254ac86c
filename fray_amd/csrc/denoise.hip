// C ABI, denoising (include/frayhip.h "denoising"): frayhip_denoise_defaults, frayhip_denoise, frayhip_denoise_signal and their _device entries.  A spatial,
// SVGF-style edge-avoiding a-trous wavelet filter of an rgb frame guided by a feature frame (frayhip_render_features).  Scene-free: it needs no
// frayhip_scene and touches none.  FP32 throughout; the Makefile builds this object with -ffp-contract=off, so every product and sum below is
// rounded where it is written (tests/denoise_ref.py restates it in numpy).
//
//   k_dn_prepare   per pixel: the guides packed for the levels (unit normal and depth; albedo; the depth gradient by central differences,
//                  one-sided at borders), the signal (rgb, or rgb / max(albedo, 1e-3) per channel) and, with rgb_half, the variance
//                  (l(c) - l(c_half))^2 prefiltered with the 3x3 binomial kernel; for frayhip_denoise_signal the caller's signal and variance as they are
//   k_dn_level     one a-trous level at step 2^k: 25 taps, edge-stopping weights, the filtered signal and its variance; the last level
//                  multiplies max(albedo, 1e-3) back and writes the output frame
// Every tap is read through L1 / L2 (no LDS tiling): at 1080p a level reads 48 bytes per tap from buffers that the neighbouring waves read too.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>

#include "entry_support.hpp"

// the B3-spline taps (1/16, 1/4, 3/8, 1/4, 1/16): all exact in FP32
static __constant__ float kB3[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};

static __device__ __forceinline__ float lum(float r, float g, float b) { return (r + g + b) / 3.0f; }      // Color::intensity, color.h:79-82
static __device__ __forceinline__ float demod1(float c, float a) { return c / fmaxf(a, 1e-3f); }

struct DenoisePrep {
    int W, H;
    const float* rgb;
    const float* half;          // null: no noise estimate
    const float* variance;      // frayhip_denoise_signal: rgb is the signal as the levels take it, this its variance; else null
    const float* feat;
    int demodulate;
    float4* g0;                 // unit normal (or 0), depth
    float4* g1;                 // albedo, 0
    float2* grad;               // depth gradient
    float4* cv;                 // signal, variance
};

// the luminance difference of the two buffers at pixel q (the signal demodulated as the filter sees it)
static __device__ __forceinline__ float half_diff(const DenoisePrep& P, size_t q)
{
    const float* c = P.rgb + 3 * q;
    const float* h = P.half + 3 * q;
    if (P.demodulate) {
        const float* a = P.feat + q * FRAYHIP_FEAT_CHANNELS + 6;
        return lum(demod1(c[0], a[0]), demod1(c[1], a[1]), demod1(c[2], a[2])) - lum(demod1(h[0], a[0]), demod1(h[1], a[1]), demod1(h[2], a[2]));
    }
    return lum(c[0], c[1], c[2]) - lum(h[0], h[1], h[2]);
}

static __global__ __launch_bounds__(256) void k_dn_prepare(DenoisePrep P)
{
    const int W = P.W, H = P.H;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
    const float* f = P.feat + p * FRAYHIP_FEAT_CHANNELS;
    float nx = f[3], ny = f[4], nz = f[5];
    const float nn = nx * nx + ny * ny + nz * nz;
    if (nn > 0.0f) {                       // a mean of several samples' normals is shorter than 1: the weights compare directions
        const float s = sqrtf(nn);
        nx = nx / s; ny = ny / s; nz = nz / s;
    }
    const float z = f[9];
    P.g0[p] = make_float4(nx, ny, nz, z);
    const float ar = f[6], ag = f[7], ab = f[8];
    P.g1[p] = make_float4(ar, ag, ab, 0.0f);
    auto depth = [&](int xx, int yy) { return P.feat[((size_t)yy * W + xx) * FRAYHIP_FEAT_CHANNELS + 9]; };
    float gx = 0.0f, gy = 0.0f;
    if (W > 1) gx = x == 0 ? depth(1, y) - z : x == W - 1 ? z - depth(W - 2, y) : (depth(x + 1, y) - depth(x - 1, y)) * 0.5f;
    if (H > 1) gy = y == 0 ? depth(x, 1) - z : y == H - 1 ? z - depth(x, H - 2) : (depth(x, y + 1) - depth(x, y - 1)) * 0.5f;
    P.grad[p] = make_float2(gx, gy);
    const float* c = P.rgb + 3 * p;
    float cr = c[0], cg = c[1], cb = c[2];
    if (P.demodulate && !P.variance) { cr = demod1(cr, ar); cg = demod1(cg, ag); cb = demod1(cb, ab); }
    float var = 0.0f;
    if (P.variance) {
        var = P.variance[p];
    } else if (P.half) {
        // 3x3 binomial (1 2 1) x (1 2 1), normalised over the taps inside the image
        float sw = 0.0f, sv = 0.0f;
        for (int j = -1; j <= 1; j++) {
            const int yy = y + j;
            if (yy < 0 || yy >= H) continue;
            for (int i = -1; i <= 1; i++) {
                const int xx = x + i;
                if (xx < 0 || xx >= W) continue;
                const float b = (i == 0 ? 2.0f : 1.0f) * (j == 0 ? 2.0f : 1.0f);
                const float dl = half_diff(P, (size_t)yy * W + xx);
                sw += b;
                sv += b * (dl * dl);
            }
        }
        var = sv / sw;
    }
    P.cv[p] = make_float4(cr, cg, cb, var);
}

struct DenoiseLevel {
    int W, H, k;
    const float4* g0;
    const float4* g1;
    const float2* grad;
    const float4* in;
    float4* next;               // null at the last level
    float* out;                 // the output frame at the last level, else null
    int demodulate, useVar;
    float sigmaL, sigmaN, sigmaZ, sigmaA;
};

static __global__ __launch_bounds__(256) void k_dn_level(DenoiseLevel L)
{
    const int W = L.W, H = L.H;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
    const int step = 1 << L.k;
    const float4 cp = L.in[p], np = L.g0[p], ap = L.g1[p];
    const float2 gp = L.grad[p];
    const bool pZero = np.x == 0.0f && np.y == 0.0f && np.z == 0.0f;
    const float lp = lum(cp.x, cp.y, cp.z);
    const float denL = L.useVar ? L.sigmaL * sqrtf(fmaxf(0.0f, cp.w)) + 1e-4f : L.sigmaL * ldexpf(1.0f, -L.k);
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    for (int j = -2; j <= 2; j++) {
        const int yq = y + j * step;
        if (yq < 0 || yq >= H) continue;
        for (int i = -2; i <= 2; i++) {
            const int xq = x + i * step;
            if (xq < 0 || xq >= W) continue;
            const size_t q = (size_t)yq * W + xq;
            const float4 cq = L.in[q], nq = L.g0[q], aq = L.g1[q];
            const float h = kB3[i + 2] * kB3[j + 2];
            const bool qZero = nq.x == 0.0f && nq.y == 0.0f && nq.z == 0.0f;
            float wn;
            if (pZero || qZero) wn = (pZero && qZero) ? 1.0f : 0.0f;
            else wn = powf(fmaxf(0.0f, np.x * nq.x + np.y * nq.y + np.z * nq.z), L.sigmaN);
            const float dz = fabsf(np.w - nq.w);
            const float wz = expf(-dz / (L.sigmaZ * fabsf(gp.x * (float)(i * step) + gp.y * (float)(j * step)) + 1e-4f));
            const float da = (fabsf(ap.x - aq.x) + fabsf(ap.y - aq.y)) + fabsf(ap.z - aq.z);
            const float wa = expf(-da / L.sigmaA);
            const float wl = expf(-fabsf(lp - lum(cq.x, cq.y, cq.z)) / denL);
            const float w = (((h * wn) * wz) * wa) * wl;
            sw += w;
            sr += w * (cq.x - cp.x);
            sg += w * (cq.y - cp.y);
            sb += w * (cq.z - cp.z);
            sv += (w * w) * cq.w;
        }
    }
    float r = cp.x, g = cp.y, b = cp.z, v = cp.w;
    if (sw > 0.0f) {                                 // the centre tap's weight; 0 only for non-finite inputs
        r = cp.x + sr / sw; g = cp.y + sg / sw; b = cp.z + sb / sw;
        v = sv / (sw * sw);
    }
    if (L.next) {
        L.next[p] = make_float4(r, g, b, v);
    } else {
        if (L.demodulate) { r = r * fmaxf(ap.x, 1e-3f); g = g * fmaxf(ap.y, 1e-3f); b = b * fmaxf(ap.z, 1e-3f); }
        float* o = L.out + 3 * p;
        o[0] = r; o[1] = g; o[2] = b;
    }
}

namespace {

using namespace frayhip_detail;

bool overlaps(const void* a, size_t an, const void* b, size_t bn)
{
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

// Every check of both entries, in this order; none touches the device.
// `variance`: the frayhip_denoise_signal entries, whose rgb is the signal and whose second buffer (W*H floats, required) is its variance.
int check(const char* who, int W, int H, const float* rgb, const float* half, const float* feat, const struct frayhip_denoise* p, const float* out, bool device,
          bool variance = false)
{
    if (W < 1 || H < 1) return bad(who, "width and height must be >= 1");
    if ((long long)W * H > (1ll << 30)) return bad(who, "more than 2^30 pixels");
    if (!rgb) return bad(who, variance ? "null signal" : "null rgb");
    if (variance && !half) return bad(who, "null variance");
    if (!feat) return bad(who, "null feat");
    if (!p) return bad(who, "null parameters");
    if (!out) return bad(who, "null out");
    if (device)
        for (const void* q : {(const void*)rgb, (const void*)half, (const void*)feat, (const void*)out})
            if (misaligned(q, 4)) return bad(who, "device pointer to floats not 4-byte aligned");
    if (p->levels < 1 || p->levels > 10) return bad(who, "levels must be 1..10");
    if (p->demodulate != 0 && p->demodulate != 1) return bad(who, "demodulate must be 0 or 1");
    const float sig[4] = {p->sigma_luminance, p->sigma_normal, p->sigma_depth, p->sigma_albedo};
    const char* names[4] = {"sigma_luminance", "sigma_normal", "sigma_depth", "sigma_albedo"};
    for (int i = 0; i < 4; i++) {
        if (!std::isfinite(sig[i]) || sig[i] < 0) return bad(who, std::string(names[i]) + " must be finite and >= 0");
        if (i != 1 && !(sig[i] > 0)) return bad(who, std::string(names[i]) + " must be > 0");
    }
    const size_t n = (size_t)W * H;
    if (overlaps(out, 12 * n, rgb, 12 * n) || overlaps(out, 12 * n, half, (variance ? 4 : 12) * n) || overlaps(out, 12 * n, feat, 4 * FRAYHIP_FEAT_CHANNELS * n))
        return bad(who, "out must not overlap an input");
    return FRAYHIP_OK;
}

struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// The device path of both entries (device pointers, checked).  Work buffers: guides, gradient and two ping-pong signal buffers, one allocation.
// `variance` as in check(): rgb and half are then the signal and its variance.
int run(const char* who, int W, int H, const float* rgb, const float* half, const float* feat, const struct frayhip_denoise* prm, float* out, hipStream_t stream,
        frayhip_stats* st, std::chrono::steady_clock::time_point t0, bool variance = false)
{
    const size_t n = (size_t)W * H;
    DeviceArrays M(std::string(who) + ": out of device memory");
    unsigned char* work;
    if (const int rc = M.alloc(work, n * (16 + 16 + 8 + 16 + 16))) return rc;
    float4* g0 = (float4*)work;
    float4* g1 = g0 + n;
    float4* cvA = g1 + n;
    float4* cvB = cvA + n;
    float2* grad = (float2*)(cvB + n);
    Events E;
    HIP_TRY(hipEventCreate(&E.a));
    HIP_TRY(hipEventCreate(&E.b));
    struct Drain { hipStream_t s; bool armed = true; ~Drain() { if (armed) (void)hipStreamSynchronize(s); } } drain{stream};
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    HIP_TRY(hipEventRecord(E.a, stream));
    hipLaunchKernelGGL(k_dn_prepare, grid, block, 0, stream, DenoisePrep{W, H, rgb, variance ? nullptr : half, variance ? half : nullptr, feat, prm->demodulate, g0, g1, grad, cvA});
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < prm->levels; k++) {
        const bool last = k == prm->levels - 1;
        const DenoiseLevel L{W, H, k, g0, g1, grad, cvA, last ? nullptr : cvB, last ? out : nullptr, prm->demodulate, half ? 1 : 0,
                      prm->sigma_luminance, prm->sigma_normal, prm->sigma_depth, prm->sigma_albedo};
        hipLaunchKernelGGL(k_dn_level, grid, block, 0, stream, L);
        HIP_TRY(hipGetLastError());
        std::swap(cvA, cvB);
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

// The host entries: host buffers copied to the device and back around run().  `variance` as in check().
int host_entry(const char* who, int width, int height, const float* rgb, const float* half, const float* feat, const struct frayhip_denoise* p, float* out,
               frayhip_stats* st, bool variance)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = check(who, width, height, rgb, half, feat, p, out, false, variance)) return rc;
    const size_t n = (size_t)width * height;
    const size_t nHalf = half ? (variance ? 1 : 3) : 0;
    // one allocation: rgb, out, feat, then rgb_half (or the variance) when given
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_rgb;
    if (const int rc = B.alloc(d_rgb, n * (3 + 3 + FRAYHIP_FEAT_CHANNELS + nHalf))) return rc;
    float* d_out = d_rgb + 3 * n;
    float* d_feat = d_out + 3 * n;
    float* d_half = half ? d_feat + FRAYHIP_FEAT_CHANNELS * n : nullptr;
    HIP_TRY(hipMemcpy(d_rgb, rgb, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_feat, feat, n * 4 * FRAYHIP_FEAT_CHANNELS, hipMemcpyHostToDevice));
    if (d_half) HIP_TRY(hipMemcpy(d_half, half, n * 4 * nHalf, hipMemcpyHostToDevice));
    if (const int rc = run(who, width, height, d_rgb, d_half, d_feat, p, d_out, nullptr, st, t0, variance)) return rc;
    HIP_TRY(hipMemcpy(out, d_out, n * 12, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

}  // namespace

extern "C" {

int frayhip_denoise_defaults(struct frayhip_denoise* p)
{
    if (!p) return bad("frayhip_denoise_defaults", "null parameters");
    p->levels = 5;
    p->demodulate = 1;
    p->sigma_luminance = 4.0f;
    p->sigma_normal = 128.0f;
    p->sigma_depth = 1.0f;
    p->sigma_albedo = 0.1f;
    return FRAYHIP_OK;
}

int frayhip_denoise_device(int width, int height, const float* d_rgb, const float* d_rgb_half, const float* d_feat, const struct frayhip_denoise* p,
                           float* d_out, void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_denoise_device";
    if (const int rc = check(who, width, height, d_rgb, d_rgb_half, d_feat, p, d_out, true)) return rc;
    return run(who, width, height, d_rgb, d_rgb_half, d_feat, p, d_out, (hipStream_t)hip_stream, st, t0);
}

int frayhip_denoise(int width, int height, const float* rgb, const float* rgb_half, const float* feat, const struct frayhip_denoise* p, float* out,
                    frayhip_stats* st)
{
    return host_entry("frayhip_denoise", width, height, rgb, rgb_half, feat, p, out, st, false);
}

int frayhip_denoise_signal_device(int width, int height, const float* d_signal, const float* d_variance, const float* d_feat, const struct frayhip_denoise* p,
                                  float* d_out, void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_denoise_signal_device";
    if (const int rc = check(who, width, height, d_signal, d_variance, d_feat, p, d_out, true, true)) return rc;
    return run(who, width, height, d_signal, d_variance, d_feat, p, d_out, (hipStream_t)hip_stream, st, t0, true);
}

int frayhip_denoise_signal(int width, int height, const float* signal, const float* variance, const float* feat, const struct frayhip_denoise* p, float* out,
                           frayhip_stats* st)
{
    return host_entry("frayhip_denoise_signal", width, height, signal, variance, feat, p, out, st, true);
}

}  // extern "C"
