// "This segment stays on one side of this triangle's plane": a certificate under which Mesh::intersectTriangle (mesh.cpp:102-141, with
// Triangle::intersectFast, triangle.cpp:66-94) on visible()'s ray (main.cpp:64-80), followed by visible()'s `info.dist < maxDist`, never makes
// visible() return false -- not in real arithmetic only, but as the reference's own code computes it, and as this project's two copies of it do
// (dev_trace.hpp tri_test / node_intersect / visible: the exact copy and the fp_contract one).  A next-event segment of a closed room starts
// 1e-6 off a wall and ends on the light: both ends lie on the inner side of every wall, so the walls' box and triangle tests (a third of
// k_pt_shadow's instructions on cornell_box) are known to report nothing nearer than the light.  k_pt_shadow evaluates the certificate for the
// planes of the scene's eligible nodes (capi.hip: untransformed meshes without a KD-tree, fewer than FRAY_GATE_MIN_TRIS triangles) and skips a node
// for a wave when every live lane certifies every triangle of it.
//
// Notation: a, b the segment's ends; L = |b - a|; d = (b - a) / L; a triangle record's N (= AB x AC as stored) and A; in REAL arithmetic
//     sigma_x = N . (x - A)       (x = a, b),        n1 = |N|_1,        S = |a|_inf + |b|_inf + |A|_inf + 1,        u = 2^-53.
// A plane entry holds N, k = fl(N . A), t1 >= c n1 and t0 >= t1 (Amax + 1) with c = 2^-36 and Amax = max |A|_inf over the triangles that share
// the entry (the host, rounding up).  The certificate holds when
//     (0)  |a|_inf + |b|_inf <= 2^100   and   |b - a|_inf >= 2^-400                     (all compares false on NaN),
//     (1)  s~_a and s~_b are both > tau~ or both < -tau~,   s~_x = fma(Nz, xz, fma(Ny, xy, fma(Nx, xx, -k))),   tau~ = fma(t1, m, t0),  m = |a|_inf + |b|_inf.
// The host admits a triangle only with finite coordinates, |A|_inf <= 2^40 and 2^-80 <= n1 <= 2^90; with (0) every product below stays between
// 2^-900 and 2^500 in magnitude or is a term whose underflow changes a sum by less than 2^-1000 of it: no overflow, no harmful underflow.
//
// Proof.  tau = c n1 S.  tau~ >= tau (1 - 3u).  s~_x differs from sigma_x by at most 8u n1 S (three fused steps on terms below n1 |x|_inf, and k
// within 3u n1 |A|_inf of N . A -- for EVERY triangle sharing the entry, whose own N . A are all within that of k).  So (1) gives, for one sign,
// which we take positive:   sigma_a >= tau',  sigma_b >= tau',   tau' = 0.99 tau.   Also sigma_x <= n1 (|x|_inf + |A|_inf) <= n1 S, and L <= 1.74 S.
//   What the code under test computes (every copy): e = fl(b - a), maxDist~ = fl |e| <= L (1 + 4u); the ray direction d~ = e normalised once (the
//   fp_contract copy) or twice (the reference: main.cpp:70 and Transform::untransformDir; an identity matrix in between adds zeros), each component
//   within a RELATIVE 16u of d's (the subtraction is componentwise exact to u, the common factor 1 / length to 6u per normalisation; (0) keeps the squares
//   normal).  Dcr~ = fl(N . -d~) is within eD = 20u n1 of Dcr = -N . d = (sigma_a - sigma_b) / L.  sg~ = fl(N . fl(a - A)) is within 4u n1 S of sigma_a,
//   hence >= 0.98 tau > 0.  gamma~ = fl(sg~ fl(1 / Dcr~)): relative error 3u on top (IEEE), below 8u with the contracted copy's refined reciprocal
//   (two ulps, dev_math.hpp) and its fused dot products, whose errors are below the ones counted here.  The budget below leaves room for 100u.
//   * |Dcr~| < 1e-12: rejected by the code itself.
//   * Dcr~ < 0: gamma~ <= -0.97 c < 0 (no underflow: sg~ >= 0.98 c n1, |1 / Dcr~| >= 1 / (2 n1)): rejected at `gamma < 0`.
//   * Dcr~ > 0 although Dcr <= 0 (the ray moves away or along, rounding flipped the sign): Dcr~ <= eD, so gamma~ >= 0.98 tau / eD (1 - 3u) > 6000 S.
//   * Dcr > 0 (the ray approaches the plane) and Dcr~ > 0: the real crossing is at t* = L + sigma_b / (N . -d) >= L + tau' / |N|_2 >= L + 0.99 c S -- b
//     itself is that far from the plane.  gamma~ >= L + c S / 2 follows from
//         (sigma_a - 4u n1 S)(1 - 100u) >= (L + c S / 2)(Dcr + eD)
//     <=  sigma_b >= 4u n1 S + 100u sigma_a + L eD + (c S / 2) Dcr + (c S / 2) eD,     with  L eD <= 35u n1 S,  Dcr <= |N|_2 <= n1:
//         the right side is below (0.5 c + 140u) n1 S = 0.501 c n1 S  <  0.99 c n1 S <= sigma_b.        (c = 2^17 u.)
//   So an accepted triangle has gamma~ >= L + c S / 2 in every case (6000 S > L + c S / 2), and a mesh whose triangles are all certified reports one of
//   its accepted gammas.  The fp_contract copy compares dist = gamma~ with maxDist~ directly: L + c S / 2 > L (1 + 4u) since c / 2 = 65536 u.  The
//   reference and the exact copy recompute dist~ = fl |a - ip|, ip = fl(a + fl(d~ gamma~)): componentwise a - ip = -gamma~ d~ up to 2u (|a_k| + gamma~),
//   so dist~ >= gamma~ (1 - 28u) - 4u S >= L + (c / 2 - 53u) S > L + 7u S >= maxDist~.  `dist < maxDist` is false.
//   * L = 0 is excluded by (0); a NaN anywhere in the code under test makes its own `dist < maxDist` false.
// The culling test, `gamma > minDist` and the barycentric tests only reject more.  BBox::testIntersect needs no argument: whether it passes or not,
// no triangle is accepted below maxDist.  NaN or infinity in a, b: (0) fails.
// tests/native/segcert_check.cpp runs the function on the host against the triangle test and the comparison restated from the reference, in both
// arithmetics, over random and adversarial segments; with the margin removed (FRAY_SEGCERT_SCALE = 0) the same harness finds contradictions.
#pragma once
#ifndef FRAY_CERT_FN
#define FRAY_CERT_FN __device__ __forceinline__
#endif
#ifndef FRAY_SEGCERT_SCALE
#define FRAY_SEGCERT_SCALE 1.0     // the harness builds a second time with 0 to show that it sees contradictions then
#endif
#define FRAY_SEG_MAX_PLANES 16     // plane entries per scene; a scene that needs more gets none
#define FRAY_SEG_MAX_NODES 16      // eligible nodes per scene
#define FRAY_SEGCERT_C 0x1p-36     // c
#define FRAY_SEGCERT_MAX_COORD 0x1p40
#define FRAY_SEGCERT_MIN_N1 0x1p-80
#define FRAY_SEGCERT_MAX_N1 0x1p90

// One plane of the table (DScene::segPlanes): what the host makes of the triangles that share it (capi.hip)
struct DSegPlane { double N[3]; double k, t0, t1; };      // 48 B

// (0): the part that depends on the segment only.  Returns m = |a|_inf + |b|_inf, or NaN when the segment cannot be certified at all.
FRAY_CERT_FN double seg_cert_scale(double ax, double ay, double az, double bx, double by, double bz, double ex, double ey, double ez)
{
    const double ma = __builtin_fmax(__builtin_fmax(__builtin_fabs(ax), __builtin_fabs(ay)), __builtin_fabs(az));
    const double mb = __builtin_fmax(__builtin_fmax(__builtin_fabs(bx), __builtin_fabs(by)), __builtin_fabs(bz));
    const double me = __builtin_fmax(__builtin_fmax(__builtin_fabs(ex), __builtin_fabs(ey)), __builtin_fabs(ez));
    // (fmax drops a NaN operand, a sum keeps it: a NaN coordinate of a or b is a NaN component of e = b - a; an infinite one fails m <= 2^100)
    const double m = ma + mb, se = ex + ey + ez;
    const bool ok = m <= 0x1p100 && me >= 0x1p-400 && se == se;
    return ok ? m : __builtin_nan("");
}

// (1) for one plane entry; m from seg_cert_scale (NaN: never certified)
FRAY_CERT_FN bool seg_same_side(double Nx, double Ny, double Nz, double k, double t0, double t1, double m,
                                double ax, double ay, double az, double bx, double by, double bz)
{
    const double sa = __builtin_fma(Nz, az, __builtin_fma(Ny, ay, __builtin_fma(Nx, ax, -k)));
    const double sb = __builtin_fma(Nz, bz, __builtin_fma(Ny, by, __builtin_fma(Nx, bx, -k)));
    const double tau = FRAY_SEGCERT_SCALE * __builtin_fma(t1, m, t0);
    return __builtin_fmin(sa, sb) > tau || __builtin_fmax(sa, sb) < -tau;
}

// host side (frayhip_scene_create, the harness): may this triangle record have a plane entry at all, and the entry of the triangles that share
// N and k = fl(N . A) bit for bit (Amax: the largest |A|_inf among them).  t1 and t0 are rounded up.
static inline bool segcert_triangle_ok(const double* N, const double* A)
{
    double n1 = 0, am = 0;
    for (int q = 0; q < 3; q++) {
        if (!(N[q] == N[q]) || !(A[q] == A[q])) return false;
        n1 += N[q] < 0 ? -N[q] : N[q];
        const double aa = A[q] < 0 ? -A[q] : A[q];
        am = am < aa ? aa : am;
    }
    return am <= FRAY_SEGCERT_MAX_COORD && n1 >= FRAY_SEGCERT_MIN_N1 && n1 <= FRAY_SEGCERT_MAX_N1;
}
static inline double segcert_offset(const double* N, const double* A) { return N[0] * A[0] + N[1] * A[1] + N[2] * A[2]; }
static inline void segcert_make(DSegPlane& o, const double* N, double k, double Amax)
{
    double n1 = 0;
    for (int q = 0; q < 3; q++) { o.N[q] = N[q]; n1 += N[q] < 0 ? -N[q] : N[q]; }
    o.k = k;
    o.t1 = FRAY_SEGCERT_C * n1 * (1.0 + 0x1p-40);
    o.t0 = o.t1 * (Amax + 1.0) * (1.0 + 0x1p-40);
}
