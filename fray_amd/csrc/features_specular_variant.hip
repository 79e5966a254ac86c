// Specular feature frames (frayhip_render_features_specular, include/frayhip.h) for one kernel flag word: the Makefile compiles this file eight
// times, -DFRAY_ST=0..5, 8, 9, into specular<ST>.o.  Objects of their own, as features<ST>.o are: k_features and the frame kernels are compiled
// exactly as they were without them.
//
//   k_features_specular<ST>
//                    k_features' loop (persistent waves claiming 8x8 tiles, the frame's camera samples 0 .. n-1, FP32 sums in sample order kept in
//                    the output row) with every sample followed through Refl / Refr nodes to the first hit that is neither, or to the bounce
//                    limit: the chain is a loop around closest_hit<ST> that a lane leaves at its terminal hit, writing its row there, and a wave
//                    when none of its lanes continues.  Carried across a search: the camera ray (o0, d0), the current ray, the path length T, the
//                    albedo product, the unfolding matrix M (nine doubles, named registers: no per-bounce array, nothing indexed) and the count b.
#include "features_specular.hpp"
#include "kernels.hpp"

#ifndef FRAY_ST
#error "compile with -DFRAY_ST=0..5, 8 or 9"
#endif

using frayhip_detail::SpecularFeatureArgs;

// Waves per SIMD.  This kernel has k_features' registers (features_variant.hip) plus 36 that live across the search (o0, d0, T, M, the product,
// b), and at k_features' figures every variant spilled (20 to 82 VGPRs).  Plain and textured words: 3 (no spill, no scratch; at 4 words 0 and 8
// spill 1 and 3).  KD words: 2 (no spill; their 236 bytes are closest_hit's KD stack, as in k_features<4>).  Cube / CSG words: 2, where the CsgOp
// machine keeps 11840 bytes per lane in scratch already and the chain adds 60 / 98 spilled VGPRs (1-1.5 % more); at 1 word 3 still spills 4.
// profiles/specular_features/README.md has each variant's count.
#ifndef FRAY_SPECULAR_WAVES
#define FRAY_SPECULAR_WAVES 3
#endif
#ifndef FRAY_SPECULAR_WAVES_KD
#define FRAY_SPECULAR_WAVES_KD 2
#endif
#ifndef FRAY_SPECULAR_WAVES_CSG
#define FRAY_SPECULAR_WAVES_CSG 2
#endif
constexpr int specular_waves(int st) { return (st & 2) ? FRAY_SPECULAR_WAVES_CSG : (st & 4) ? FRAY_SPECULAR_WAVES_KD : FRAY_SPECULAR_WAVES; }

// shader_albedo of features_variant.hip, restated: that file is an object of its own and stays the code it is.  The colour the shader's shade()
// starts from (include/frayhip.h "feature frames"); D: Layered shaders that may still be entered below this one.
template <int ST, int D>
FD C3 terminal_albedo(const DScene& S, int shader, V3 d, const HitInfo& info, Cnt& c)
{
    const FRAY_RO DShader& sh = S.shaders[shader];
    if (sh.kind == 1 || sh.kind == 2) {
        C3 a = ldc(sh.color);
        if (sh.texture >= 0) a = a * texture_sample<ST>(S, sh.texture, d, info, c);
        return a;
    }
    if (sh.kind == 3 || sh.kind == 4) return ldc(sh.mult);
    if (sh.kind == 0) return ldc(sh.color);
    C3 result = c3(0, 0, 0);
    if constexpr (D > 0) {
        for (int i = 0; i < sh.layerCount; i++) {
            const FRAY_RO DLayer& Ly = S.layers[sh.layerBegin + i];
            const C3 opacity = Ly.texture >= 0 ? texture_sample<ST>(S, Ly.texture, d, info, c) : ldc(Ly.opacity);
            result = terminal_albedo<ST, D - 1>(S, Ly.shader, d, info, c) * opacity + (c3(1, 1, 1) - opacity) * result;
        }
    }
    return result;
}

// spawn_ray's generator argument for the two shaders that draw nothing (Reflection / Refraction::spawnRay)
struct NoDraw {};
FD double rng_double(NoDraw&) { return 0.0; }

template <int ST>
static __global__ __launch_bounds__(256, specular_waves(ST)) void k_features_specular(SpecularFeatureArgs A)
{
    Cnt c = zero_cnt();
    const int nItems = A.nItems;
    DCursors* const cur = A.cur;
    for (int r = 0, item = claim_items(cur, nItems, r); item < nItems; item = claim_items(cur, nItems, r)) {
        const FRAY_RO SpecularFeatureArgs* AP = kernel_args<SpecularFeatureArgs>();
        const DScene& S = KARG(SpecularFeatureArgs, AP, S);
        const DCamera& C = KARG(SpecularFeatureArgs, AP, C);
        const DFrame& F = KARG(SpecularFeatureArgs, AP, F);
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        const int n = KARG(SpecularFeatureArgs, AP, n);
        const uint32_t p = (uint32_t)y * (uint32_t)F.W + (uint32_t)x;
        // the running FP32 sums live in the output rows themselves, as k_features' do: sample 0 stores, the others add
        float* const out = KARG(SpecularFeatureArgs, AP, feat) + (size_t)p * FRAYHIP_FEAT_CHANNELS;
        float* const bo = KARG(SpecularFeatureArgs, AP, bounces);          // null: no plane asked for
        for (int i = 0; i < n; i++) {
            // the camera sample, exactly k_features'
            float ox, oy;
            V3 o, d;
            if (F.jitter) {                                                               // gi or DOF
                Mt tab = mt_seed(sample_seed(F.seed, p, (uint32_t)i)), rnd = tab;
                ox = rng_float(rnd); oy = rng_float(rnd);
                const double fx = (double)((float)x + ox), fy = (double)((float)y + oy);   // int + float, main.cpp:359
                if (C.dof) dof_ray(C, fx, fy, tab, o, d); else screen_ray(C, fx, fy, o, d);
                if (tab.j > 227) c.envelope = 1;                                         // the lens drew past the register stream's words
            } else {                                                                      // Whitted: the AA offsets (sample 0: none)
                ox = (float)kAAOffsets[i][0]; oy = (float)kAAOffsets[i][1];
                screen_ray(C, (double)((float)x + ox), (double)((float)y + oy), o, d);
            }
            bump<ST>(c.samples);
            // the chain's state
            const V3 o0 = o, d0 = d;
            double T = 0.0;
            C3 prod = c3(1, 1, 1);                                                        // read only once b > 0
            double m00 = 1, m01 = 0, m02 = 0, m10 = 0, m11 = 1, m12 = 0, m20 = 0, m21 = 0, m22 = 1;
            int b = 0;
            for (;;) {
                HitT<ST> h;
                closest_hit<ST>(S, o, d, h, c);
                V3 ip = v3(0, 0, 0), norm = v3(0, 0, 0);
                double depth = 0;
                C3 alb;
                if (h.node >= 0) {
                    const FRAY_RO DNode& N = S.nodes[h.node];
                    const FRAY_RO DShader& sh = S.shaders[N.shader];
                    HitInfo info;
                    finalize_hit<ST>(S, h, o, d, sh.usesUV || N.bumpTex >= 0, info);
                    apply_bump<ST>(S, h.node, info, c);
                    if ((sh.kind == 3 || sh.kind == 4) && b < KARG(SpecularFeatureArgs, AP, maxBounces)) {
                        // the path tracer's own next ray; a Refr under total internal reflection comes back with pdf 1 and is the terminal
                        PathRay in, next;
                        in.o = o; in.d = d; in.depth = 0; in.flags = 0;
                        NoDraw none;
                        C3 brdf;
                        float pdf;
                        spawn_ray(sh, info, in, none, next, brdf, pdf);
                        if (sh.kind == 3 || pdf != 1.0f) {
                            const C3 mult = ldc(sh.mult);
                            prod = b == 0 ? mult : prod * mult;
                            T = T + h.dist;
                            if (sh.kind == 3) {                                           // M <- M (I - 2 m m^T)
                                const V3 m = info.norm;
                                const double u0 = (m00 * m.x + m01 * m.y) + m02 * m.z;
                                const double u1 = (m10 * m.x + m11 * m.y) + m12 * m.z;
                                const double u2 = (m20 * m.x + m21 * m.y) + m22 * m.z;
                                m00 = m00 - (2 * u0) * m.x; m01 = m01 - (2 * u0) * m.y; m02 = m02 - (2 * u0) * m.z;
                                m10 = m10 - (2 * u1) * m.x; m11 = m11 - (2 * u1) * m.y; m12 = m12 - (2 * u1) * m.z;
                                m20 = m20 - (2 * u2) * m.x; m21 = m21 - (2 * u2) * m.y; m22 = m22 - (2 * u2) * m.z;
                            }
                            o = next.o; d = next.d;
                            b = b + 1;
                            continue;
                        }
                    }
                    ip = info.ip; norm = info.norm; depth = h.dist;
                    alb = terminal_albedo<ST, 2>(S, N.shader, d, info, c);
                } else if (h.node <= -2) {
                    const FRAY_RO DLight& L = S.lights[-2 - h.node];
                    light_record(L, o, d, ip, norm);
                    depth = h.dist;
                    alb = ldc(L.color);
                } else {
                    alb = environment<ST>(S, d, c);
                }
                // the terminal's row: b == 0 k_features' own; behind a chain the virtual hit (a miss keeps its zeros)
                if (b > 0) {
                    alb = prod * alb;
                    if (h.node != -1) {
                        depth = T + h.dist;
                        ip = o0 + d0 * depth;
                        const V3 q = norm;
                        norm = v3((m00 * q.x + m01 * q.y) + m02 * q.z, (m10 * q.x + m11 * q.y) + m12 * q.z, (m20 * q.x + m21 * q.y) + m22 * q.z);
                    }
                }
                const float v[FRAYHIP_FEAT_CHANNELS] = {(float)ip.x, (float)ip.y, (float)ip.z, (float)norm.x, (float)norm.y, (float)norm.z,
                                                        alb.r, alb.g, alb.b, (float)depth};
#pragma unroll
                for (int k = 0; k < FRAYHIP_FEAT_CHANNELS; k++) out[k] = i == 0 ? v[k] : out[k] + v[k];
                if (bo) bo[p] = i == 0 ? (float)b : bo[p] + (float)b;
                break;
            }
        }
        if (n > 1) {
            const float fn = (float)n;
#pragma unroll
            for (int k = 0; k < FRAYHIP_FEAT_CHANNELS; k++) out[k] = out[k] / fn;
            if (bo) bo[p] = bo[p] / fn;
        }
    }
    if (ST & 1) flush_stats(A.st, c);
    if (c.envelope) atomicAdd(&A.st->rngOverflow, 1ull);
}

namespace frayhip_detail {
template <int ST> void launch_features_specular(hipStream_t stream, const SpecularFeatureArgs& A)
{
    const dim3 grid(persistent_grid((size_t)A.nItems, specular_waves(ST)));
    hipLaunchKernelGGL((k_features_specular<ST>), grid, dim3(256), 0, stream, A);
}
template void launch_features_specular<FRAY_ST>(hipStream_t, const SpecularFeatureArgs&);
}  // namespace frayhip_detail
