// Feature frames (frayhip_render_features, frayhip_render_features_motion, include/frayhip.h) for one kernel flag word: the Makefile compiles this file eight times,
// -DFRAY_ST=0..5, 8, 9, into features<ST>.o.  Objects of their own: the frame kernels of render_variant.hip are compiled exactly as they were
// without them (kernels.hpp is not touched, only included here once more).
//
//   k_features<ST, MOTION>
//                    per pixel of the frame's buckets, the first hit of the frame's camera samples 0 .. n-1 (k_pt_init's / k_whitted's film
//                    position and camera or thin-lens ray, same seed), the hit's position, normal after the bump, albedo and depth, summed in
//                    FP32 in sample order and divided by n; persistent waves claiming 8x8 tiles as k_primary does.  MOTION: a second row per pixel,
//                    where the hit point and its normal were in the previous frame's state of the scene (the hit node's previous transform), summed
//                    the same way.  MOTION = false is the kernel as it was: the motion code is compiled out, not branched over.
#include "features.hpp"
#include "kernels.hpp"

#ifndef FRAY_ST
#error "compile with -DFRAY_ST=0..5, 8 or 9"
#endif

using frayhip_detail::DPrevXform;
using frayhip_detail::FeatureArgs;

// Waves per SIMD: k_query_closest's (query_variant.hip), whose loop this is with a camera ray in front and the record's shading behind, except in
// the Cube / CSG variants: at their 3 waves the albedo's texture and Layered code on top of the CsgOp machine spilled 79 / 132 VGPRs (the record's
// kernel: 77 / 113); at 2 none.
#ifndef FRAY_FEATURE_WAVES_KD
#define FRAY_FEATURE_WAVES_KD 3
#endif
#ifndef FRAY_FEATURE_WAVES_CSG
#define FRAY_FEATURE_WAVES_CSG 2
#endif
constexpr int features_waves(int st) { return (st & 2) ? FRAY_FEATURE_WAVES_CSG : st == 4 ? FRAY_FEATURE_WAVES_KD : primary_waves(st); }

// The colour the shader's shade() starts from (include/frayhip.h "feature frames"): Lambert / Phong color times the diffuse texture's sample,
// Refl / Refr mult, Const color, Layered the blend of Layered::shade (shading.cpp:357-367) over its layers' albedos.  D: Layered shaders that
// may still be entered below this one; past that a Layered layer counts as black.
template <int ST, int D>
FD C3 shader_albedo(const DScene& S, int shader, V3 d, const HitInfo& info, Cnt& c)
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
            result = shader_albedo<ST, D - 1>(S, Ly.shader, d, info, c) * opacity + (c3(1, 1, 1) - opacity) * result;
        }
    }
    return result;
}

template <int ST, bool MOTION>
static __global__ __launch_bounds__(256, features_waves(ST)) void k_features(FeatureArgs A)
{
    Cnt c = zero_cnt();
    const int nItems = A.nItems;
    DCursors* const cur = A.cur;
    for (int r = 0, item = claim_items(cur, nItems, r); item < nItems; item = claim_items(cur, nItems, r)) {
        const FRAY_RO FeatureArgs* AP = kernel_args<FeatureArgs>();
        const DScene& S = KARG(FeatureArgs, AP, S);
        const DCamera& C = KARG(FeatureArgs, AP, C);
        const DFrame& F = KARG(FeatureArgs, AP, F);
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        const int n = KARG(FeatureArgs, AP, n);
        const uint32_t p = (uint32_t)y * (uint32_t)F.W + (uint32_t)x;
        // the running FP32 sums live in the output row itself (no register holds them across the search): sample 0 stores, the others add
        float* const out = KARG(FeatureArgs, AP, feat) + (size_t)p * FRAYHIP_FEAT_CHANNELS;
        for (int i = 0; i < n; i++) {
            // the camera sample: k_pt_init / k_whitted's film position and ray.  Both generators start from the sample's seed; the jitter draws
            // from one, the lens from the other (a copy made before the jitter).  Frames that draw nothing here need no seed.
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
                ip = info.ip; norm = info.norm; depth = h.dist;
                alb = shader_albedo<ST, 2>(S, N.shader, d, info, c);
            } else if (h.node <= -2) {
                const FRAY_RO DLight& L = S.lights[-2 - h.node];
                light_record(L, o, d, ip, norm);
                depth = h.dist;
                alb = ldc(L.color);
            } else {
                alb = environment<ST>(S, d, c);
            }
            const float v[FRAYHIP_FEAT_CHANNELS] = {(float)ip.x, (float)ip.y, (float)ip.z, (float)norm.x, (float)norm.y, (float)norm.z,
                                                    alb.r, alb.g, alb.b, (float)depth};
#pragma unroll
            for (int k = 0; k < FRAYHIP_FEAT_CHANNELS; k++) out[k] = i == 0 ? v[k] : out[k] + v[k];
            if constexpr (MOTION) {
                // where this point of the hit node was in the previous state: Transform::untransformPoint of the node's transform now, then
                // transformPoint of its previous one; the normal goes the way Node::intersect carries one (through m, not rescaled).  Only the
                // lanes whose node moved read the table; everything else repeats the feature row's position and normal.
                float mv = 0.0f;
                if (h.node >= 0) {
                    if (KARG(FeatureArgs, AP, moved)[h.node]) {
                        const FRAY_RO DNode& N = S.nodes[h.node];
                        const DPrevXform& X = KARG(FeatureArgs, AP, prev)[h.node];
                        ip = mulM(mulM(ip - ld3(N.T.off), N.T.inv), X.m) + ld3(X.off);
                        norm = mulM(mulM(norm, N.T.inv), X.m);
                        mv = 1.0f;
                    }
                }
                // the sums live in the motion row, as the feature sums live in theirs
                float* const mo = KARG(FeatureArgs, AP, motion) + (size_t)p * FRAYHIP_MOTION_CHANNELS;
                const float w[FRAYHIP_MOTION_CHANNELS] = {(float)ip.x, (float)ip.y, (float)ip.z, mv, (float)norm.x, (float)norm.y, (float)norm.z, 0.0f};
#pragma unroll
                for (int k = 0; k < FRAYHIP_MOTION_CHANNELS; k++) mo[k] = i == 0 ? w[k] : mo[k] + w[k];
            }
        }
        if (n > 1) {
            const float fn = (float)n;
#pragma unroll
            for (int k = 0; k < FRAYHIP_FEAT_CHANNELS; k++) out[k] = out[k] / fn;
            if constexpr (MOTION) {
                float* const mo = KARG(FeatureArgs, AP, motion) + (size_t)p * FRAYHIP_MOTION_CHANNELS;
#pragma unroll
                for (int k = 0; k < FRAYHIP_MOTION_CHANNELS; k++) mo[k] = mo[k] / fn;
            }
        }
    }
    if (ST & 1) flush_stats(A.st, c);
    if (c.envelope) atomicAdd(&A.st->rngOverflow, 1ull);
}

namespace frayhip_detail {
template <int ST> void launch_features(hipStream_t stream, const FeatureArgs& A, bool motion)
{
    const dim3 grid(persistent_grid((size_t)A.nItems, features_waves(ST)));
    if (motion) hipLaunchKernelGGL((k_features<ST, true>), grid, dim3(256), 0, stream, A);
    else hipLaunchKernelGGL((k_features<ST, false>), grid, dim3(256), 0, stream, A);
}
template void launch_features<FRAY_ST>(hipStream_t, const FeatureArgs&, bool);
}  // namespace frayhip_detail
