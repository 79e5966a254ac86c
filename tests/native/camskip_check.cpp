// Test harness (CPU) of tests/test_camera_skip_host.py: the certificate of fray_amd/csrc/dev_gatecert.hpp on FLAT meshes -- two-triangle quads, the walls whose miss
// records the first bounce skips by (dev_trace.hpp camera_skip_nodes).  tests/native/gatecert_check.cpp runs the same certificate on closed blocks; a quad's box
// has zero extent in one axis (an axis-aligned one) or is nearly empty (an oblique one), and its margin there is the whole of hf: that harness never looked at
// such a box.  Restated from the reference as there: Mesh::intersect's brute-force loop over Mesh::intersectTriangle / Triangle::intersectFast on the local ray of
// an untransformed node (the direction normalised once more), without the culling test and the mesh's box test, which can only remove hits; and the fp_contract
// copy of the device code (one normalisation, fused products).  A mesh counts as hit when either restatement accepts a triangle.
// Meshes: the five walls of the Cornell box as scenes/cornell/*.obj give them (floor, ceiling, back wall, right wall, left wall; the floor and the left wall are
// no rectangles, the left wall is not planar), each cut along either diagonal; generated quads at scales 1e-2 .. 1e3: axis-aligned rectangles, oblique
// parallelograms, planar quads that are no parallelograms.
// Rays: random ones; from outside through the edges and corners of the quad at offsets from 1e-9 (and from a rounding error) up to the quad's size; nearly
// parallel to its plane, slopes around the record's guard threshold and from 1e-13 to 1e-2, beside, above and in the plane; starting on the plane (inside and
// outside the quad, exactly, 1e-9 off, a rounding off) in any direction, in-plane ones among them; exact zeros in the direction with a start at the plane's own
// coordinate; the camera's: from (278, 273, -800) k through a point of the wall's plane near its outline.
// Exit code 1 if a certified ray has a triangle accepted, a wall or a generated rectangle gets no record, or nothing was certified (a vacuous run).  Built a second
// time with -DFRAY_GATECERT_SCALE=0 -DFRAY_MISSCERT_SCALE=0 (no margins, no guard) the same harness must find contradictions.
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
// the quad a b c d cut along a-c (diag 0) or b-d (diag 1)
static Mesh quad(V a, V b, V c, V d, int diag)
{
    Mesh M;
    if (diag == 0) { add_tri(M, a, b, c); add_tri(M, a, c, d); }
    else { add_tri(M, b, c, d); add_tri(M, b, d, a); }
    M.lo = {1e300, 1e300, 1e300}; M.hi = {-1e300, -1e300, -1e300};
    for (V p : {a, b, c, d}) {
        M.lo = {fmin(M.lo.x, p.x), fmin(M.lo.y, p.y), fmin(M.lo.z, p.z)};
        M.hi = {fmax(M.hi.x, p.x), fmax(M.hi.y, p.y), fmax(M.hi.z, p.z)};
    }
    M.size = length(M.hi - M.lo);
    return M;
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

static uint64_t rs = 0xD1B54A32D192ED03ULL;
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

int main(int argc, char** argv)
{
    const long N = argc > 1 ? atol(argv[1]) : 2000000;
    // ---- the five walls (scenes/cornell/*.obj, faces "f 4 3 2 1"), either diagonal
    const V wall[5][4] = {
        {{3.2, 0, 0}, {556, 0, 0}, {556, 0, 559.2}, {6.4, 0, 559.2}},                     // floor
        {{0, 548.8, 0}, {0, 548.8, 559.2}, {556, 548.8, 559.2}, {556, 548.8, 0}},         // ceiling
        {{6.4, 0, 559.2}, {556, 0, 559.2}, {556, 548.8, 559.2}, {0, 548.8, 559.2}},       // back wall
        {{556, 0, 559.2}, {556, 0, 0}, {556, 548.8, 0}, {556, 548.8, 559.2}},             // right wall
        {{3.2, 0, 0}, {6.4, 0, 559.2}, {0, 548.8, 559.2}, {0, 548.8, 0}},                 // left wall
    };
    static const char* const wallName[5] = {"floor", "ceiling", "back wall", "right wall", "left wall"};
    std::vector<Mesh> fixed;
    int refusedWrongly = 0;
    for (int w = 0; w < 5; w++)
        for (int diag = 0; diag < 2; diag++) {
            fixed.push_back(quad(wall[w][3], wall[w][2], wall[w][1], wall[w][0], diag));
            DGateTight F;
            if (!make_record(fixed.back(), F)) { fprintf(stderr, "the %s (diagonal %d) got no record\n", wallName[w], diag); refusedWrongly++; continue; }
            printf("%s, diagonal %d: guard %.4g, %d direction(s), half extents %.6g %.6g %.6g\n", wallName[w], diag, F.guard, F.nDirs, F.hf[0], F.hf[1], F.hf[2]);
        }
    const int nKinds = 4, nModes = 7;
    long cases = 0, certified = 0, hits = 0, bad = 0, perMode[nModes] = {0}, certMode[nModes] = {0}, badMode[nModes] = {0}, boxOnly = 0, guardBack = 0, meshes = 0, refusedRandom = 0;
    long certKind[nKinds] = {0}, perKind[nKinds] = {0};
    double guardMin = 1e300, guardMax = 0;
    Mesh M;
    DGateTight G;
    int kind = 0;
    for (long it = 0; it < N; it++) {
        if (it % 64 == 0) {               // a new mesh
            kind = pick(nKinds);
            if (kind == 0) M = fixed[pick((int)fixed.size())];
            else {
                const double sc = pick(3) == 0 ? 1e-2 : pick(2) ? 1.0 : 1e3;
                const V c = V{sym(), sym(), sym()} * (sc * mag(-1, 1.5));
                const double a = sc * mag(-0.3, 0.3), b = sc * mag(-0.3, 0.3);
                V ex, ey;
                if (kind == 1) { const int k = pick(3); const V e[3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}; ex = e[(k + 1) % 3]; ey = e[(k + 2) % 3]; }      // axis-aligned: zero extent in axis k
                else { ex = unit(); ey = normalized(cross(ex, unit())); if (kind == 2 && pick(2)) ey = normalized(ey + ex * sym() * 0.5); }           // oblique (a sheared one: a parallelogram)
                const double s1 = kind == 3 ? 0.6 + u01() : 1.0, s2 = kind == 3 ? 0.6 + u01() : 1.0;                                                   // no parallelogram
                M = quad(c, c + ex * a, c + ex * (a * s1) + ey * (b * s2), c + ey * b, pick(2));
            }
            if (!make_record(M, G)) {
                // (a generated quad may be too elongated for the guard's cap: refused rightly, and skipped; the walls and plain rectangles of aspect below 4 must be admitted)
                if (kind <= 1) { fprintf(stderr, "an admissible quad (kind %d) was refused\n", kind); refusedWrongly++; } else refusedRandom++;
                it += 63; continue;
            }
            meshes++;
            guardMin = fmin(guardMin, G.guard); guardMax = fmax(guardMax, G.guard);
        }
        const Tri& T = M.t[pick(2)];
        const V n = normalized(T.N);
        const double size = M.size;
        const V centre = (M.lo + M.hi) * 0.5;
        const double Mx = fmax(fmax(fabs(M.lo.x), fabs(M.hi.x)), fmax(fmax(fabs(M.lo.y), fabs(M.hi.y)), fmax(fabs(M.lo.z), fabs(M.hi.z))));
        auto inTri = [&](double u, double v) { return T.A + T.AB * u + T.AC * v; };
        auto around = [&](double r) { return centre + V{sym(), sym(), sym()} * (size * r); };
        auto margin = [&](V s) { return 1e-5 + 0x1p-21 * (fmax(fabs(s.x), fmax(fabs(s.y), fabs(s.z))) + Mx); };
        auto outline = [&]() {          // a point on the triangle's outline: a corner one time in three
            const int e = pick(3);
            const double w = pick(3) == 0 ? (double)pick(2) : u01();
            return e == 0 ? inTri(w, 0) : e == 1 ? inTri(0, w) : inTri(w, 1 - w);
        };
        V s, q;
        const int mode = pick(nModes);
        if (mode == 0) { s = around(mag(-1, 1)); q = pick(2) ? unit() : around(0.7) - s; }
        else if (mode == 1) {
            // from outside through an edge or a corner: offsets from 1e-9 up to the quad's size, around the margin, and down to a rounding error
            s = centre + unit() * (size * mag(0.2, 1.5));
            const int ok = pick(4);
            const double off = ok == 0 ? mag(-9, -4) : ok == 1 ? margin(s) * mag(-2, 2) : ok == 2 ? size * mag(-16, -9) : size * mag(-4, 0);
            q = outline() + unit() * off - s;
            if (pick(2)) q = normalized(q);
        } else if (mode == 2) {
            // nearly parallel to the plane: a direction in it plus n * eps, eps around the record's guard threshold (|nf . d| against Gf |d|_1) or from 1e-13 to 1e-2
            const V t = normalized(T.AB * sym() + T.AC * sym());
            const double eps = sgn() * (pick(2) ? (double)G.guard * mag(-1.5, 1.5) : mag(-13, -2));
            const V p = inTri(u01() * 3 - 1, u01() * 3 - 1);
            const int hk = pick(4);
            const double h = hk == 0 ? 0.0 : hk == 1 ? margin(p) * mag(-2, 2) : hk == 2 ? size * mag(-14, -8) : size * mag(-4, 0);
            s = p + n * (sgn() * h) - t * (size * (pick(2) ? mag(-2, 1) : 0.0));
            q = t + n * eps;
        } else if (mode == 3) {
            // starts on the plane: inside the quad or beside it; exactly, 1e-9 off, a rounding off; any direction, or one in the plane
            const int hk = pick(3);
            s = inTri(u01() * 3 - 1, u01() * 3 - 1) + n * (hk == 0 ? 0.0 : hk == 1 ? sgn() * mag(-9, -5) : sgn() * size * mag(-16, -10));
            q = pick(3) ? unit() : T.AB * sym() + T.AC * sym();
            if (pick(4) == 0) q = outline() - s;
        } else if (mode == 4) {
            // exact zeros in the direction; the start at the box's own coordinates one time in two (a flat box: the plane's)
            s = around(mag(-1, 1));
            if (pick(2)) { const int k = pick(3); (&s.x)[k] = pick(2) ? (&M.lo.x)[k] : (&M.hi.x)[k]; }
            const int k = pick(3), k2 = (k + 1 + pick(2)) % 3;
            double v[3] = {0, 0, 0};
            v[k] = sgn() * mag(-2, 2);
            if (pick(2)) v[k2] = sgn() * mag(-2, 2);
            q = {v[0], v[1], v[2]};
        } else if (mode == 5) {
            // the camera's: from where the Cornell camera stands against this quad's box, through a point of the plane near the outline (a tile's rays fan out
            // by 1e-3 of the distance) or anywhere in the box's neighbourhood
            s = centre + V{0.0, -0.003, -1.93} * size + V{sym(), sym(), sym()} * (size * 0.3);
            q = (pick(2) ? outline() + unit() * (size * mag(-6, -1)) : around(0.8)) - s;
            q = normalized(q);
        } else {
            // unnormalised segments towards the plane
            s = around(mag(-1, 1));
            q = (inTri(u01() * 1.4 - 0.2, u01() * 1.4 - 0.2) + unit() * (margin(s) * mag(-2, 3)) - s) * (pick(3) == 0 ? mag(-3, 3) : 1.0);
        }
        cases++; perMode[mode]++; perKind[kind]++;
        const float ox = (float)s.x, oy = (float)s.y, oz = (float)s.z, dx = (float)q.x, dy = (float)q.y, dz = (float)q.z;
        const float omax = fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz)), dsum = fabsf(dx) + fabsf(dy) + fabsf(dz);
        const bool boxPart = ray_surely_misses_box_f32(G.cf[0], G.cf[1], G.cf[2], G.hf[0], G.hf[1], G.hf[2], G.Mf, ox, oy, oz, dx, dy, dz, omax, dsum) && omax < 1e9f;
        const bool cert = ray_surely_misses_mesh_f32(G, ox, oy, oz, dx, dy, dz, omax, dsum);          // (the three parts camera_skip_nodes evaluates)
        if (boxPart) boxOnly++;
        if (boxPart && !cert) guardBack++;
        const bool hr = ref_hit(M, s, q), hc = contracted_hit(M, s, q);
        if (hr || hc) hits++;
        if (cert) {
            certified++; certMode[mode]++; certKind[kind]++;
            if (hr || hc) {
                if (bad < 10) fprintf(stderr, "CONTRADICTION (mode %d, kind %d, %s): certified, but a triangle accepts the ray\n  s %.17g %.17g %.17g\n  q %.17g %.17g %.17g\n  box %.17g %.17g %.17g .. %.17g %.17g %.17g\n",
                                      mode, kind, hr ? "reference" : "contracted copy", s.x, s.y, s.z, q.x, q.y, q.z, M.lo.x, M.lo.y, M.lo.z, M.hi.x, M.hi.y, M.hi.z);
                bad++; badMode[mode]++;
            }
        }
    }
    printf("cases %ld, hit %ld, certified %ld (%.1f %% of the cases), contradictions %ld\n", cases, hits, certified, 100.0 * certified / (cases ? cases : 1), bad);
    printf("certified per mode:");
    for (int k = 0; k < nModes; k++) printf(" %d: %ld/%ld", k, certMode[k], perMode[k]);
    printf("\ncertified per kind (walls, axis-aligned, oblique, no parallelogram):");
    for (int k = 0; k < nKinds; k++) printf(" %ld/%ld", certKind[k], perKind[k]);
    printf("\ncontradictions per mode:");
    for (int k = 0; k < nModes; k++) printf(" %d: %ld", k, badMode[k]);
    printf("\nbox part passed %ld, of which the guard sent back %ld; guard thresholds %.3g .. %.3g\n", boxOnly, guardBack, guardMin, guardMax);
    printf("meshes %ld, generated ones refused %ld, refused wrongly %d\n", meshes, refusedRandom, refusedWrongly);
    bool vacuous = hits == 0;
    for (int k = 0; k < nKinds; k++) vacuous = vacuous || certKind[k] == 0;
    if (vacuous) fprintf(stderr, "a vacuous run: no hit at all, or a kind of mesh without a certified ray\n");
    return (bad || refusedWrongly || vacuous) ? 1 : 0;
}
