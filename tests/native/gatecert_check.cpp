// Test harness (CPU) of tests/test_gatecert_host.py: fray_amd/csrc/dev_gatecert.hpp -- "this ray surely misses this mesh: none of its triangles accepts it" --
// against what the certificate speaks about, restated below from the reference: Mesh::intersect's brute-force loop (mesh.cpp:157-161) over
// Mesh::intersectTriangle / Triangle::intersectFast (mesh.cpp:102-141, triangle.cpp:66-94) on the local ray of an untransformed node (Node::intersect
// normalises the direction once more, geometry.cpp:196-208), without the culling test and without the mesh's box test, which can only remove hits.
// The fp_contract copy of the device code is restated too (one normalisation, fused products), and a mesh counts as hit when either restatement
// accepts a triangle.
// Meshes: the two blocks of a Cornell box (five faces each), boxes rotated and scaled (1e-2 .. 1e3) anywhere, an L-shaped prism (not convex), a box around
// the origin; a box with a sliver, a hexagonal pyramid (seven normal directions), a mesh with a NaN and one with a wrong stored normal must be refused.
// Rays: random ones; aimed at edges and corners of the triangles at distances around the margin; nearly parallel to a face (1e-13 .. 1e-2, on both
// sides of the guard threshold), beside, above and inside it; starts far away; starts on the faces; axis-parallel directions; unnormalised segment
// directions; the Cornell situation (starts 1e-6 above the floor beside a block, aimed at a light or anywhere); NaN and infinity.
// Exit code 1 if a certified ray has a triangle accepted, or an inadmissible mesh gets a record, or a NaN / infinite ray is certified.  Built a second
// time with -DFRAY_GATECERT_SCALE=0 -DFRAY_MISSCERT_SCALE=0 (no margins, no guard) the same harness must find contradictions, near-parallel ones among them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define FRAY_CERT_FN static inline
#include "dev_gatecert.hpp"

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
struct Mesh { std::vector<Tri> t; V lo, hi; double size; };

static void add_tri(Mesh& M, V a, V b, V c) { Tri T; T.A = a; T.AB = b - a; T.AC = c - a; T.N = cross(T.AB, T.AC); M.t.push_back(T); }
static void add_quad(Mesh& M, V a, V b, V c, V d) { add_tri(M, a, b, c); add_tri(M, a, c, d); }
static void finish(Mesh& M)
{
    M.lo = {1e300, 1e300, 1e300}; M.hi = {-1e300, -1e300, -1e300};
    for (const Tri& T : M.t)
        for (int c = 0; c < 3; c++) {
            const V p = c == 0 ? T.A : c == 1 ? T.A + T.AB : T.A + T.AC;
            M.lo = {fmin(M.lo.x, p.x), fmin(M.lo.y, p.y), fmin(M.lo.z, p.z)};
            M.hi = {fmax(M.hi.x, p.x), fmax(M.hi.y, p.y), fmax(M.hi.z, p.z)};
        }
    M.size = length(M.hi - M.lo);
}

// the reference's loop: does any triangle accept the ray (s, q)?  (info.dist starts at INF and only shrinks: `gamma > best` rejects more)
static bool ref_hit(const Mesh& M, V s, V q)
{
    const V d = normalized(normalized(q)), D = -d;
    double best = 1e99;
    bool found = false;
    for (const Tri& T : M.t) {
        const double Dcr = dot(T.N, D);
        if (fabs(Dcr) < 1e-12) continue;
        const double rDcr = 1 / Dcr;
        const V H = s - T.A;
        const double gamma = dot(T.N, H) * rDcr;
        if (gamma < 0 || gamma > best) continue;
        const double l2 = dot(cross(H, T.AC), D) * rDcr;
        if (l2 < 0 || l2 > 1) continue;
        const double l3 = dot(cross(T.AB, H), D) * rDcr;
        if (l3 < 0 || l3 > 1) continue;
        if (1 - (l2 + l3) < 0) continue;
        best = gamma; found = true;
    }
    return found;
}
// the device's fp_contract copy: one normalisation, fused products
static bool contracted_hit(const Mesh& M, V s, V q)
{
    const V d = q * (1.0 / sqrt(fdot(q, q))), D = -d;
    double best = 1e99;
    bool found = false;
    for (const Tri& T : M.t) {
        const double Dcr = fdot(T.N, D);
        if (fabs(Dcr) < 1e-12) continue;
        const double rDcr = 1 / Dcr;
        const V H = s - T.A;
        const double gamma = fdot(T.N, H) * rDcr;
        if (gamma < 0 || gamma > best) continue;
        const V hc = {fma(H.y, T.AC.z, -(H.z * T.AC.y)), fma(H.z, T.AC.x, -(H.x * T.AC.z)), fma(H.x, T.AC.y, -(H.y * T.AC.x))};
        const double l2 = fdot(hc, D) * rDcr;
        if (l2 < 0 || l2 > 1) continue;
        const V bh = {fma(T.AB.y, H.z, -(T.AB.z * H.y)), fma(T.AB.z, H.x, -(T.AB.x * H.z)), fma(T.AB.x, H.y, -(T.AB.y * H.x))};
        const double l3 = fdot(bh, D) * rDcr;
        if (l3 < 0 || l3 > 1) continue;
        if (1 - (l2 + l3) < 0) continue;
        best = gamma; found = true;
    }
    return found;
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

static bool make_record(const Mesh& M, DGateTight& G)
{
    std::vector<GateTri> gt;
    for (const Tri& T : M.t) gt.push_back(GateTri{&T.A.x, &T.AB.x, &T.AC.x, &T.N.x});
    return gatecert_make(G, gt.data(), (int)gt.size());
}

// a box with the corners c + (+-ex) + (+-ey) + (+-ez); `open`: without its bottom (-ey) face, as the Cornell blocks are
static Mesh box_mesh(V c, V ex, V ey, V ez, bool open)
{
    Mesh M;
    auto P = [&](int i, int j, int k) { return c + ex * (i ? 1.0 : -1.0) + ey * (j ? 1.0 : -1.0) + ez * (k ? 1.0 : -1.0); };
    add_quad(M, P(0, 1, 0), P(0, 1, 1), P(1, 1, 1), P(1, 1, 0));
    if (!open) add_quad(M, P(0, 0, 0), P(1, 0, 0), P(1, 0, 1), P(0, 0, 1));
    add_quad(M, P(0, 0, 0), P(0, 1, 0), P(1, 1, 0), P(1, 0, 0));
    add_quad(M, P(0, 0, 1), P(1, 0, 1), P(1, 1, 1), P(0, 1, 1));
    add_quad(M, P(0, 0, 0), P(0, 0, 1), P(0, 1, 1), P(0, 1, 0));
    add_quad(M, P(1, 0, 0), P(1, 1, 0), P(1, 1, 1), P(1, 0, 1));
    finish(M);
    return M;
}
// a Cornell block from its four top corners, standing on the floor (its sides are not quite parallel: five normal directions)
static Mesh cornell_block(const double top[4][2], double h)
{
    Mesh M;
    V t[4], b[4];
    for (int i = 0; i < 4; i++) { t[i] = {top[i][0], h, top[i][1]}; b[i] = {top[i][0], 0, top[i][1]}; }
    add_quad(M, t[0], t[1], t[2], t[3]);
    for (int i = 0; i < 4; i++) add_quad(M, b[i], b[(i + 1) % 4], t[(i + 1) % 4], t[i]);
    finish(M);
    return M;
}
static void frame(V& ex, V& ey, V& ez)
{
    ex = unit();
    ey = normalized(cross(ex, unit()));
    ez = cross(ex, ey);
}
static Mesh l_prism(V c, V ex, V ey, V ez)          // an L: the square [-1, 1]^2 without its (+, +) quarter, extruded along ey
{
    Mesh M;
    const double px[6] = {-1, 1, 1, 0, 0, -1}, pz[6] = {-1, -1, 0, 0, 1, 1};
    auto P = [&](int i, double y) { return c + ex * px[i] + ey * y + ez * pz[i]; };
    for (double y : {-1.0, 1.0}) { add_quad(M, P(0, y), P(1, y), P(2, y), P(3, y)); add_quad(M, P(0, y), P(3, y), P(4, y), P(5, y)); }
    for (int i = 0; i < 6; i++) add_quad(M, P(i, -1), P((i + 1) % 6, -1), P((i + 1) % 6, 1), P(i, 1));
    finish(M);
    return M;
}

int main(int argc, char** argv)
{
    const long N = argc > 1 ? atol(argv[1]) : 2000000;
    int refusedWrongly = 0, admittedWrongly = 0;
    long refusedRandom = 0, meshes = 0;
    // ---- meshes that must be refused
    {
        DGateTight G;
        Mesh S = box_mesh({10, 5, 3}, {2, 0, 0}, {0, 1, 0}, {0, 0, 3}, false);
        add_tri(S, {10, 5, 3}, {14, 5, 3}, {12, 5 + 1e-7, 3});                                         // a sliver
        if (make_record(S, G)) { fprintf(stderr, "a mesh with a sliver got a record\n"); admittedWrongly++; }
        Mesh Py;                                                                                       // a hexagonal pyramid: seven normal directions
        const V apex = {0.3, 3, 0.1};
        V ring[6];
        for (int i = 0; i < 6; i++) ring[i] = {2 * cos(1.0 + i), 0, 2 * sin(1.0 + i)};
        for (int i = 0; i < 6; i++) add_tri(Py, ring[i], ring[(i + 1) % 6], apex);
        for (int i = 1; i < 5; i++) add_tri(Py, ring[0], ring[i], ring[i + 1]);
        if (make_record(Py, G)) { fprintf(stderr, "a pyramid of seven directions got a record\n"); admittedWrongly++; }
        Mesh Nn = box_mesh({1, 2, 3}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, false);
        Nn.t[3].A.y = NAN;
        if (make_record(Nn, G)) { fprintf(stderr, "a mesh with a NaN got a record\n"); admittedWrongly++; }
        Mesh Wn = box_mesh({1, 2, 3}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, false);
        Wn.t[2].N = Wn.t[2].N * 1.001 + V{1e-3, 0, 0};
        if (make_record(Wn, G)) { fprintf(stderr, "a mesh with a wrong stored normal got a record\n"); admittedWrongly++; }
        Mesh Big = box_mesh({1e8, 2, 3}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, false);
        if (make_record(Big, G)) { fprintf(stderr, "a mesh at 1e8 got a record\n"); admittedWrongly++; }
        if (G.tight || G.nDirs || G.guard != 0) { fprintf(stderr, "a refused record is not zeroed\n"); admittedWrongly++; }
    }
    // ---- the fixed meshes
    const double shortTop[4][2] = {{426, 65}, {474, 225}, {316, 272}, {266, 114}}, tallTop[4][2] = {{133, 247}, {291, 296}, {242, 456}, {84, 406}};
    std::vector<Mesh> fixed;
    fixed.push_back(cornell_block(shortTop, 165));
    fixed.push_back(cornell_block(tallTop, 330));
    fixed.push_back(box_mesh({0.3, -0.2, 0.1}, {2, 0, 0}, {0, 1.5, 0}, {0, 0, 1}, false));             // its box holds the origin
    for (int k = 0; k < 3; k++) { DGateTight F; if (make_record(fixed[k], F)) printf("fixed mesh %d: guard %.3g, %d directions, half extents %.6g %.6g %.6g\n", k, F.guard, F.nDirs, F.hf[0], F.hf[1], F.hf[2]); }
    const int nKinds = 6, nModes = 9;
    long cases = 0, certified = 0, hits = 0, bad = 0, badNonFinite = 0, perMode[nModes] = {0}, certMode[nModes] = {0}, badMode[nModes] = {0}, boxOnly = 0, guardBack = 0;
    double guardMin = 1e300, guardMax = 0;
    Mesh M;
    DGateTight G;
    for (long it = 0; it < N; it++) {
        if (it % 64 == 0) {               // a new mesh
            const int kind = pick(nKinds);
            if (kind < 3) M = fixed[kind];
            else {
                const double sc = pick(3) == 0 ? 1e-2 : pick(2) ? 1.0 : 1e3;
                V ex, ey, ez;
                frame(ex, ey, ez);
                const V c = V{sym(), sym(), sym()} * (sc * mag(-1, 1.5));
                if (kind == 3) M = box_mesh(c, ex * (sc * mag(-0.3, 0.3)), ey * (sc * mag(-0.3, 0.3)), ez * (sc * mag(-0.3, 0.3)), pick(2) != 0);
                else if (kind == 4) M = l_prism(c, ex * (sc * mag(-0.3, 0.3)), ey * (sc * mag(-0.3, 0.3)), ez * (sc * mag(-0.3, 0.3)));
                else M = box_mesh(c, V{1, 0, 0} * (sc * mag(-0.3, 0.3)), V{0, 1, 0} * (sc * mag(-0.3, 0.3)), V{0, 0, 1} * (sc * mag(-0.3, 0.3)), pick(2) != 0);    // axis-aligned
            }
            // (a random box may be too elongated for the guard's cap: refused rightly, and skipped; the fixed meshes must be admitted)
            if (!make_record(M, G)) { if (kind < 3) { fprintf(stderr, "an admissible mesh (kind %d) was refused\n", kind); refusedWrongly++; } else refusedRandom++; it += 63; continue; }
            meshes++;
            guardMin = fmin(guardMin, G.guard); guardMax = fmax(guardMax, G.guard);
        }
        const Tri& T = M.t[pick((int)M.t.size())];
        const V n = normalized(T.N);
        const double size = M.size;
        const V centre = (M.lo + M.hi) * 0.5;
        const double Mx = fmax(fmax(fabs(M.lo.x), fabs(M.hi.x)), fmax(fmax(fabs(M.lo.y), fabs(M.hi.y)), fmax(fabs(M.lo.z), fabs(M.hi.z))));
        auto inTri = [&](double u, double v) { return T.A + T.AB * u + T.AC * v; };
        auto around = [&](double r) { return centre + V{sym(), sym(), sym()} * (size * r); };
        auto margin = [&](V s) { return 1e-5 + 0x1p-21 * (fmax(fabs(s.x), fmax(fabs(s.y), fabs(s.z))) + Mx); };
        V s, q;
        const int mode = pick(nModes);
        if (mode == 0) { s = around(mag(-1, 1)); q = pick(2) ? unit() : around(0.7) - s; }
        else if (mode == 1) {
            // aimed at an edge or a corner of the triangle, passing it at a distance around the margin (or around the coordinates' rounding)
            const int e = pick(3);
            const double w = pick(3) == 0 ? (double)pick(2) : u01();
            const V onEdge = e == 0 ? inTri(w, 0) : e == 1 ? inTri(0, w) : inTri(w, 1 - w);
            s = pick(4) ? around(mag(-0.5, 1)) : around(mag(1, 4));
            const double off = pick(3) ? margin(s) * mag(-2, 2) : size * mag(-16, -9);
            q = onEdge + unit() * off - s;
        } else if (mode == 2) {
            // nearly parallel to the face: a direction in its plane plus n * eps, eps from 1e-13 to 1e-2; the line passes beside, above or through the face
            const V t = normalized(T.AB * sym() + T.AC * sym());
            const double eps = sgn() * mag(-13, -2);
            const V p = inTri(u01() * 3 - 1, u01() * 3 - 1);
            const int hk = pick(4);
            const double h = hk == 0 ? 0.0 : hk == 1 ? margin(p) * mag(-2, 2) : hk == 2 ? size * mag(-14, -8) : size * mag(-4, 0);
            s = p + n * (sgn() * h) - t * (size * (pick(2) ? mag(-2, 1) : 0.0));
            q = t + n * eps;
        } else if (mode == 3) {
            s = centre + unit() * (size * mag(2, 6));
            q = around(pick(2) ? 0.6 : 2.0) - s;
            if (pick(2)) q = normalized(q);
        } else if (mode == 4) {
            // starts on a face, 1e-6 off it, or a rounding off it; any direction
            const int hk = pick(3);
            s = inTri(u01(), u01() * 0.999) + n * (hk == 0 ? 0.0 : hk == 1 ? sgn() * 1e-6 : sgn() * size * mag(-16, -10));
            q = unit();
        } else if (mode == 5) {
            // exact zeros in the direction
            s = around(mag(-1, 1));
            if (pick(3) == 0) s = inTri(u01(), u01()) + unit() * (size * mag(-8, 0));
            const int k = pick(3), k2 = (k + 1 + pick(2)) % 3;
            double v[3] = {0, 0, 0};
            v[k] = sgn() * mag(-2, 2);
            if (pick(2)) v[k2] = sgn() * mag(-2, 2);
            q = {v[0], v[1], v[2]};
        } else if (mode == 6) {
            // unnormalised segments: b - a with lengths from 1e-3 to 1e3 of the mesh
            s = around(mag(-1, 1));
            const V b = pick(2) ? around(mag(-1, 1)) : inTri(u01() * 1.4 - 0.2, u01() * 1.4 - 0.2) + unit() * (margin(s) * mag(-2, 3));
            q = (b - s) * (pick(3) == 0 ? mag(-3, 3) : 1.0);
        } else if (mode == 7) {
            s = around(1); q = unit();
            const double badv = pick(2) ? NAN : sgn() * INFINITY;
            double* w = pick(2) ? &s.x : &q.x;
            w[pick(3)] = badv;
        } else {
            // the Cornell situation: a start just above the floor the mesh stands on (its lowest y), beside or under it, aimed anywhere upwards or at a light overhead
            s = {centre.x + sym() * size, M.lo.y + (pick(2) ? 1e-6 : size * mag(-9, -3)), centre.z + sym() * size};
            if (pick(2)) { q = unit(); q.y = fabs(q.y); }
            else q = V{centre.x + sym() * size * 0.3, M.hi.y + size * (0.2 + u01()), centre.z + sym() * size * 0.3} - s;
        }
        cases++; perMode[mode]++;
        const float ox = (float)s.x, oy = (float)s.y, oz = (float)s.z, dx = (float)q.x, dy = (float)q.y, dz = (float)q.z;
        const float omax = fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz)), dsum = fabsf(dx) + fabsf(dy) + fabsf(dz);
        const bool boxPart = ray_surely_misses_box_f32(G.cf[0], G.cf[1], G.cf[2], G.hf[0], G.hf[1], G.hf[2], G.Mf, ox, oy, oz, dx, dy, dz, omax, dsum) && omax < 1e9f;
        const bool cert = ray_surely_misses_mesh_f32(G, ox, oy, oz, dx, dy, dz, omax, dsum) && omax < 1e9f;          // (ray_gate_class's own last line)
        if (boxPart) boxOnly++;
        if (boxPart && !cert) guardBack++;
        if (mode == 7) { if (cert) { badNonFinite++; fprintf(stderr, "a ray with a NaN or an infinity was certified\n"); } continue; }
        const bool hr = ref_hit(M, s, q), hc = contracted_hit(M, s, q);
        if (hr || hc) hits++;
        if (cert) {
            certified++; certMode[mode]++;
            if (hr || hc) {
                if (bad < 10) fprintf(stderr, "CONTRADICTION (mode %d, %s): certified, but a triangle accepts the ray\n  s %.17g %.17g %.17g\n  q %.17g %.17g %.17g\n  box %.17g %.17g %.17g .. %.17g %.17g %.17g\n",
                                      mode, hr ? "reference" : "contracted copy", s.x, s.y, s.z, q.x, q.y, q.z, M.lo.x, M.lo.y, M.lo.z, M.hi.x, M.hi.y, M.hi.z);
                bad++; badMode[mode]++;
            }
        }
    }
    printf("cases %ld, hit %ld, certified %ld (%.1f %% of the cases), contradictions %ld\n", cases, hits, certified, 100.0 * certified / (cases ? cases : 1), bad);
    printf("certified per mode:");
    for (int k = 0; k < nModes; k++) printf(" %d: %ld/%ld", k, certMode[k], perMode[k]);
    printf("\ncontradictions per mode:");
    for (int k = 0; k < nModes; k++) printf(" %d: %ld", k, badMode[k]);
    printf("\nbox part passed %ld, of which the guard sent back %ld; guard thresholds %.3g .. %.3g\n", boxOnly, guardBack, guardMin, guardMax);
    printf("meshes %ld, random ones refused %ld\n", meshes, refusedRandom);
    printf("meshes refused wrongly %d, admitted wrongly %d, non-finite rays certified %ld\n", refusedWrongly, admittedWrongly, badNonFinite);
    return (bad || refusedWrongly || admittedWrongly || badNonFinite) ? 1 : 0;
}
