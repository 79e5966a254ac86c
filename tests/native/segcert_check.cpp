// Test harness (CPU): fray_amd/csrc/dev_segcert.hpp -- "this segment stays on one side of this triangle's plane, so the triangle cannot occlude it" --
// against what the certificate speaks about, restated below from the reference: visible() (main.cpp:64-80) for one untransformed mesh node of one
// triangle, i.e. the ray made from the segment, Node::intersect's second normalisation (geometry.cpp:196-208 with an identity transform),
// Triangle::intersectFast (triangle.cpp:66-94), the hit point and `info.dist < maxDist`.  The fp_contract copy of the device code is restated too
// (one normalisation, fused dot products, dist = gamma), and a case counts as occluded when either restatement says so.  The box test is left out:
// it can only remove hits.
// Segments: random ones; ends at offsets around tau on either side of the plane; nearly parallel to the plane (|Dcr| from 1e-20 to 1e-6); in the plane of
// a triangle that lies elsewhere; ending just short of and just beyond the triangle; coordinates scaled by 1e-3, 1 and 1e4; exact zeros in the direction;
// degenerate lengths.  Exit code 1 if a certified segment is reported occluded.  Built a second time with -DFRAY_SEGCERT_SCALE=0 the same harness
// must find contradictions (it then tests a certificate without a margin).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define FRAY_CERT_FN static inline
#include "dev_segcert.hpp"

struct V { double x, y, z; };
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator-(V a) { return {-a.x, -a.y, -a.z}; }
static V operator*(V a, double m) { return {a.x * m, a.y * m, a.z * m}; }
static double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static double length(V a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
static V normalized(V a) { double m = 1.0 / length(a); return a * m; }              // vector.h:81-85
static double fdot(V a, V b) { return fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)); }     // a dot product as a contracting compiler may fuse it

struct Tri { V A, AB, AC, N; };

// the reference: is the segment a..b occluded by the triangle?
static bool ref_occluded(const Tri& T, V a, V b)
{
    V dir = b - a;
    const double maxDist = length(a - b);           // distance(a, b)
    dir = normalized(dir);                          // ray.dir.normalize()
    const V s = a, d = normalized(dir);             // untransformPoint / untransformDir of an identity transform
    const V D = -d;
    const double Dcr = dot(T.N, D);
    if (fabs(Dcr) < 1e-12) return false;
    const double rDcr = 1 / Dcr;
    const V H = s - T.A;
    const double gamma = dot(T.N, H) * rDcr;
    if (gamma < 0 || gamma > 1e99) return false;    // minDist = INF (mesh.cpp:153)
    const double l2 = dot(cross(H, T.AC), D) * rDcr;
    if (l2 < 0 || l2 > 1) return false;
    const double l3 = dot(cross(T.AB, H), D) * rDcr;
    if (l3 < 0 || l3 > 1) return false;
    if (1 - (l2 + l3) < 0) return false;
    const V ip = s + d * gamma;                     // mesh.cpp:112; transformPoint of an identity transform
    const double dist = length(a - ip);             // geometry.cpp:206
    return dist < maxDist;
}
// the device's fp_contract copy (dev_trace.hpp with FRAY_ARITH: one normalisation, fused products, the ray parameter is the distance)
static bool contracted_occluded(const Tri& T, V a, V b)
{
    const V e = b - a;
    const double maxDist = sqrt(fdot(e, e));
    const V d = e * (1.0 / maxDist), D = -d;
    const double Dcr = fdot(T.N, D);
    if (fabs(Dcr) < 1e-12) return false;
    const double rDcr = 1 / Dcr;
    const V H = a - T.A;
    const double gamma = fdot(T.N, H) * rDcr;
    if (gamma < 0 || gamma > 1e99) return false;
    const V hc = {fma(H.y, T.AC.z, -(H.z * T.AC.y)), fma(H.z, T.AC.x, -(H.x * T.AC.z)), fma(H.x, T.AC.y, -(H.y * T.AC.x))};
    const double l2 = fdot(hc, D) * rDcr;
    if (l2 < 0 || l2 > 1) return false;
    const V bh = {fma(T.AB.y, H.z, -(T.AB.z * H.y)), fma(T.AB.z, H.x, -(T.AB.x * H.z)), fma(T.AB.x, H.y, -(T.AB.y * H.x))};
    const double l3 = fdot(bh, D) * rDcr;
    if (l3 < 0 || l3 > 1) return false;
    if (1 - (l2 + l3) < 0) return false;
    return gamma < maxDist;
}

static uint64_t rs = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
static double u01() { return (rnd() >> 11) * (1.0 / 9007199254740992.0); }
static double sym() { return 2 * u01() - 1; }
static double mag(double lo, double hi) { return pow(10.0, lo + (hi - lo) * u01()); }
static int pick(int n) { return (int)(rnd() % (uint64_t)n); }
static double sgn() { return pick(2) ? 1.0 : -1.0; }
static V unit()
{
    for (;;) { V d = {sym(), sym(), sym()}; double l = sqrt(dot(d, d)); if (l > 1e-3 && l <= 1) return d * (1.0 / l); }
}

int main(int argc, char** argv)
{
    const long N = argc > 1 ? atol(argv[1]) : 2000000;
    long cases = 0, certified = 0, occluded = 0, bad = 0, perMode[10] = {0}, certMode[10] = {0};
    for (long it = 0; it < N; it++) {
        const double scales[3] = {1e-3, 1.0, 1e4};
        const double sc = scales[pick(3)];
        // the triangle: axis-aligned walls (exact zeros in N), tilted ones, slivers
        Tri T;
        T.A = V{sym(), sym(), sym()} * (sc * mag(-1, 1));
        const int shape = pick(4);
        if (shape == 0) {               // a wall in a coordinate plane, like the Cornell box's
            const int k = pick(3);
            const double w = sc * mag(-1, 1), h = sc * mag(-1, 1);
            T.AB = k == 0 ? V{0, w, 0} : k == 1 ? V{0, 0, w} : V{w, 0, 0};
            T.AC = k == 0 ? V{0, 0, h} : k == 1 ? V{h, 0, 0} : V{0, h, 0};
        } else if (shape == 1) {        // a sliver
            T.AB = unit() * (sc * mag(-1, 1));
            T.AC = T.AB * mag(-1, 0) + unit() * (sc * mag(-6, -2));
        } else {
            T.AB = unit() * (sc * mag(-2, 1));
            T.AC = unit() * (sc * mag(-2, 1));
        }
        T.N = cross(T.AB, T.AC);
        const double Nv[3] = {T.N.x, T.N.y, T.N.z}, Av[3] = {T.A.x, T.A.y, T.A.z};
        if (!segcert_triangle_ok(Nv, Av)) continue;
        DSegPlane P;
        segcert_make(P, Nv, segcert_offset(Nv, Av), fmax(fabs(Av[0]), fmax(fabs(Av[1]), fabs(Av[2]))));
        const double nl = length(T.N);
        const V n = T.N * (1.0 / nl);
        const double n1 = fabs(T.N.x) + fabs(T.N.y) + fabs(T.N.z);
        auto inTri = [&](double u, double v) { return T.A + T.AB * u + T.AC * v; };
        auto somewhere = [&]() { return T.A + V{sym(), sym(), sym()} * (sc * mag(-2, 1.5)); };
        // distance from the plane that corresponds to tau for points of this size
        auto tauDist = [&](V a, V b) {
            const double S = fmax(fabs(a.x), fmax(fabs(a.y), fabs(a.z))) + fmax(fabs(b.x), fmax(fabs(b.y), fabs(b.z))) + fmax(fabs(Av[0]), fmax(fabs(Av[1]), fabs(Av[2]))) + 1;
            return FRAY_SEGCERT_C * n1 * S / nl;
        };
        V a, b;
        const int mode = pick(9);
        if (mode == 0) { a = somewhere(); b = somewhere(); }                      // random
        else if (mode == 1) {
            // ends at offsets around tau on either side of the plane, the chord passing through (or near) the triangle
            const V pa = inTri(u01() * 1.2 - 0.1, u01() * 1.2 - 0.1) + (T.AB * sym() + T.AC * sym()) * mag(-3, 0.5);
            const V pb = inTri(u01() * 1.2 - 0.1, u01() * 1.2 - 0.1);
            const double t = tauDist(pa, pb);
            a = pa + n * (sgn() * t * mag(-2, 2));
            b = pb + n * (sgn() * t * mag(-2, 2));
        } else if (mode == 2) {
            // nearly parallel to the plane: |Dcr| / |N| from 1e-20 to 1e-6, both ends on one side at heights around tau up to the triangle's size
            const V pa = inTri(sym() * 2, sym() * 2), pb = inTri(u01(), u01());
            const double L = length(pb - pa), t = tauDist(pa, pb), side = sgn();
            const double ha = pick(2) ? t * mag(-1, 3) : sc * mag(-6, 0);
            a = pa + n * (side * ha);
            b = pb + n * (side * (ha - sgn() * L * mag(-20, -6)));
        } else if (mode == 3) {
            // in the plane of a triangle that lies elsewhere (coplanar, disjoint) -- or a hair off it
            const V pa = inTri(2 + u01() * 3, 2 + u01() * 3), pb = inTri(-2 - u01() * 3, 2 + u01() * 3);
            const double off = pick(3) == 0 ? 0.0 : sgn() * tauDist(pa, pb) * mag(-3, 2);
            a = pa + n * off; b = pb + n * (pick(2) ? off : -off);
        } else if (mode == 4 || mode == 5) {
            // aimed through the triangle from one side, ending just short of (4) or just beyond (5) it
            const V hit = inTri(u01() * 0.45 + 0.02, u01() * 0.45 + 0.02);
            const double side = sgn();
            a = hit + n * (side * sc * mag(-3, 1)) + (T.AB * sym() + T.AC * sym()) * mag(-2, 0.3);
            const V dir = hit - a;
            // (offsets around tau, and down to the rounding of the coordinates: what a certificate without a margin gets wrong)
            const double t = tauDist(a, hit), over = (pick(2) ? t * mag(-3, 3) : t * mag(-9, -3)) / fmax(fabs(dot(normalized(dir), n)), 1e-30);
            b = hit + normalized(dir) * (mode == 4 ? -over : over);
        } else if (mode == 6) {
            // exact zeros in the direction: the segment runs along a coordinate axis (or in a coordinate plane)
            a = somewhere();
            b = a;
            const int k = pick(3);
            const double step = sgn() * sc * mag(-3, 1.5);
            if (k == 0) b.x += step; else if (k == 1) b.y += step; else b.z += step;
            if (pick(2)) { const int k2 = (k + 1) % 3; const double s2 = sgn() * sc * mag(-3, 1.5); if (k2 == 0) b.x += s2; else if (k2 == 1) b.y += s2; else b.z += s2; }
        } else if (mode == 7) {
            // degenerate lengths: a == b, b one ulp from a, lengths down to 1e-300
            a = pick(2) ? somewhere() : inTri(u01(), u01()) + n * (sgn() * tauDist(T.A, T.A) * mag(-1, 3));
            const int w = pick(3);
            if (w == 0) b = a;
            else if (w == 1) b = {nextafter(a.x, pick(2) ? 1e300 : -1e300), a.y, pick(2) ? a.z : nextafter(a.z, 1e300)};
            else b = a + unit() * mag(-300, -10);
        } else {
            // the Cornell situation: a start 1e-6 (scaled or not) off the plane, the end far from it on the same side -- or, wrongly, on the other
            const V pa = inTri(u01() * 1.5 - 0.25, u01() * 1.5 - 0.25);
            const double side = sgn();
            a = pa + n * (side * (pick(2) ? 1e-6 : 1e-6 * sc) * mag(-1, 1));
            b = inTri(u01(), u01()) + n * ((pick(4) ? side : -side) * sc * mag(-2, 1)) + T.AB * sym() + T.AC * sym();
        }
        cases++; perMode[mode]++;
        const V e = b - a;
        const double m = seg_cert_scale(a.x, a.y, a.z, b.x, b.y, b.z, e.x, e.y, e.z);
        const bool cert = seg_same_side(P.N[0], P.N[1], P.N[2], P.k, P.t0, P.t1, m, a.x, a.y, a.z, b.x, b.y, b.z);
        const bool occR = ref_occluded(T, a, b), occC = contracted_occluded(T, a, b);
        if (occR || occC) occluded++;
        if (cert) {
            certified++; certMode[mode]++;
            if (occR || occC) {
                if (bad < 10) fprintf(stderr, "CONTRADICTION (mode %d, %s): certified, but the triangle occludes the segment\n  A %.17g %.17g %.17g\n  AB %.17g %.17g %.17g\n  AC %.17g %.17g %.17g\n  a %.17g %.17g %.17g\n  b %.17g %.17g %.17g\n",
                                      mode, occR ? "reference" : "contracted copy", T.A.x, T.A.y, T.A.z, T.AB.x, T.AB.y, T.AB.z, T.AC.x, T.AC.y, T.AC.z, a.x, a.y, a.z, b.x, b.y, b.z);
                bad++;
            }
        }
    }
    printf("cases %ld, occluded %ld, certified %ld (%.1f %% of the cases), contradictions %ld\n", cases, occluded, certified, 100.0 * certified / (cases ? cases : 1), bad);
    printf("certified per mode:");
    for (int k = 0; k < 9; k++) printf(" %d: %ld/%ld", k, certMode[k], perMode[k]);
    printf("\n");
    return bad ? 1 : 0;
}
