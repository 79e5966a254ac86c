// Test harness (CPU) of tests/test_camera_tiles_host.py: the first bounce's tile certificate (fray_amd/csrc/dev_camtile.hpp) and the tile table's pixel origin.
// usage: camtile_check N SCENE.fray ...          the certificate, N tiles
//        camtile_check --origin                  the table's origin against item_pixel and frayhip_bucket_xy
//
// The certificate.  Every scene file is parsed with the product's parser and run through arena_build; every miss record of its table (DCamSkip) is taken with the
// triangles of its node's mesh from the description.  For cameras and 8x8 pixel tiles of the classes below, every (tile, record) pair the certificate passes is
// held to the mesh's triangle loop: rays made exactly as screen_ray (kernels.hpp) makes them -- the tile's pixels inside the frame, jitter 0, 0x1.fffffep-1f (the
// float sum then rounds to px + 1: the rectangle's far edge) and random, the four corners of the rectangle among them -- must not be accepted by any triangle of
// the mesh.  A pair whose box part the tile passes and whose guard it does not is an ASKED one (dev_camtile.hpp): of its rays those that pass the per-ray form's guard and
// bounds, in FP32 as dev_trace.hpp camera_guard_nodes evaluates them, must not be accepted either; it counts as refused below.  The loop is restated from the reference as tests/native/camskip_check.cpp and gatecert_check.cpp restate it: Mesh::intersect's brute-force loop over
// Mesh::intersectTriangle / Triangle::intersectFast on the local ray of an untransformed node (the direction normalised once more), without the culling test and
// the mesh's box test, which can only remove hits; and the fp_contract copy of the device code (one normalisation, fused products).
// Cameras are the product's (capi.hip camera_begin_frame restated: three rotations, fov, aspect); a class that needs a ray through a chosen point moves the
// camera's position along that ray, which leaves the directions alone.
//   0  random cameras inside and outside the room, fov 10 .. 120, random tiles
//   1  a corner ray of the tile passes an edge or a corner of the mesh at 1e-4 .. 1e-9 (and at a rounding error)
//   2  the tile straddles a silhouette: a ray inside the rectangle passes through a point of the outline, or up to three tile widths beside it
//   3  the camera in the plane of a face (exactly, 1e-9 off, a rounding off), inside the face or beside it
//   4  the camera inside the mesh's box
//   5  directions at the guard threshold: the tile looks along a face, slopes around the record's guard; and far below it, crossing the plane beside the outline
//   6  frames whose size is no multiple of 8: the tiles of the ragged right and bottom edges
// Every class must certify some pairs and refuse some (a class that certifies nothing tests nothing): exit code 1 otherwise, or if a certified pair has a ray
// accepted.  Built a second time with -DFRAY_CAMTILE_SCALE=0 -DFRAY_GATECERT_SCALE=0 -DFRAY_MISSCERT_SCALE=0 (no margins, no guard, and the records' half extents
// no longer rounded up: load() below) the same harness must find contradictions.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define FRAY_CERT_FN static inline
#include "host_scene.h"
#include "scene_arena.hpp"
#include "dev_camtile.hpp"

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
struct Mesh { std::vector<Tri> t; V lo, hi; double size; DCamSkip rec; std::string name; };

// the reference's loop: does any triangle accept the ray (s, q)?  (info.dist starts at INF and only shrinks: `gamma > best` rejects more)
static bool ref_hit(const Mesh& M, V s, V q)
{
    const V d = normalized(q), D = -d;
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

// capi.hip camera_begin_frame (Camera::beginFrame), the part screen_ray reads
static void rowmul(const double* v, const double* m, double* o) { for (int j = 0; j < 3; j++) o[j] = v[0] * m[j] + v[1] * m[3 + j] + v[2] * m[6 + j]; }
static void matmul3(const double* a, const double* b, double* c)
{
    for (int i = 0; i < 9; i++) c[i] = 0.0;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) c[i * 3 + j] += a[i * 3 + k] * b[k * 3 + j];
}
static DCamera camera(double yaw, double pitch, double roll, double fov, double aspect, int W, int H)
{
    const double PI = 3.141592653589793238;
    auto rad = [&](double a) { return a / 180.0 * PI; };
    DCamera f;
    memset(&f, 0, sizeof f);
    const double lenBC = sqrt(aspect * aspect + 1.0);
    const double m = tan(rad(fov / 2)) / lenBC;
    const double tl[3] = {-aspect * m, +m, 1}, tr[3] = {+aspect * m, +m, 1}, bl[3] = {-aspect * m, -m, 1};
    double S, C;
    sincos(rad(roll), &S, &C);
    const double rz[9] = {C, -S, 0, S, C, 0, 0, 0, 1};
    sincos(rad(pitch), &S, &C);
    const double rx[9] = {1, 0, 0, 0, C, -S, 0, S, C};
    sincos(rad(yaw), &S, &C);
    const double ry[9] = {C, 0, S, 0, 1, 0, -S, 0, C};
    double t[9], rot[9];
    matmul3(rz, rx, t);
    matmul3(t, ry, rot);
    rowmul(tl, rot, f.topLeft); rowmul(tr, rot, f.topRight); rowmul(bl, rot, f.bottomLeft);
    f.w = W; f.h = H;
    return f;
}
// a camera whose image centre looks along `front` (any frame about it)
static DCamera camera_along(V front, double fov, double aspect, int W, int H)
{
    DCamera f;
    memset(&f, 0, sizeof f);
    const V fr = normalized(front), rt = normalized(cross(unit(), fr)), up = cross(fr, rt);
    const double m = tan(fov / 360.0 * 3.141592653589793238) / sqrt(aspect * aspect + 1.0);
    const V tl = fr + up * m - rt * (aspect * m), tr = fr + up * m + rt * (aspect * m), bl = fr - up * m - rt * (aspect * m);
    f.topLeft[0] = tl.x; f.topLeft[1] = tl.y; f.topLeft[2] = tl.z;
    f.topRight[0] = tr.x; f.topRight[1] = tr.y; f.topRight[2] = tr.z;
    f.bottomLeft[0] = bl.x; f.bottomLeft[1] = bl.y; f.bottomLeft[2] = bl.z;
    f.w = W; f.h = H;
    return f;
}
// kernels.hpp screen_ray, operation for operation
static void screen_ray(const DCamera& C, double x, double y, V& o, V& d)
{
    const V tl = {C.topLeft[0], C.topLeft[1], C.topLeft[2]}, tr = {C.topRight[0], C.topRight[1], C.topRight[2]}, bl = {C.bottomLeft[0], C.bottomLeft[1], C.bottomLeft[2]};
    d = tl + (tr - tl) * (x / C.w) + (bl - tl) * (y / C.h);
    d = normalized(d);
    o = {C.pos[0], C.pos[1], C.pos[2]};
}
static V raw_dir(const DCamera& C, double x, double y)
{
    const V tl = {C.topLeft[0], C.topLeft[1], C.topLeft[2]}, tr = {C.topRight[0], C.topRight[1], C.topRight[2]}, bl = {C.bottomLeft[0], C.bottomLeft[1], C.bottomLeft[2]};
    return tl + (tr - tl) * (x / C.w) + (bl - tl) * (y / C.h);
}
static void set_pos(DCamera& C, V p) { C.pos[0] = p.x; C.pos[1] = p.y; C.pos[2] = p.z; }

static int load(const char* path, std::vector<Mesh>& out)
{
    std::string err;
    frayhost::HostScene* hs = frayhost::parse_scene_file(path, err);
    if (!hs) { fprintf(stderr, "%s: %s\n", path, err.c_str()); return 2; }
    frayhip_arena::ArenaBuilt B;
    frayhip_arena::arena_build(hs->desc, B);
    const DCamSkip* R = (const DCamSkip*)(B.host.data() + B.tables[B.F.tCamSkip].off);
    const frayhip_scene_desc& d = hs->desc;
    for (int r = 0; r < B.F.nCamSkip; r++) {
        const frayhip_node& N = d.nodes[R[r].node];
        const frayhip_mesh& m = d.meshes[d.geoms[N.geom].index];
        Mesh M;
        M.rec = R[r];
        M.name = std::string(path) + " node " + std::to_string(R[r].node);
        M.lo = {1e300, 1e300, 1e300}; M.hi = {-1e300, -1e300, -1e300};
        for (int t = 0; t < m.n_triangles; t++) {
            Tri T;
            const double* a = &m.vertices[3 * (size_t)m.triangles[t].v[0]];
            T.A = {a[0], a[1], a[2]};
            T.AB = {m.triangles[t].AB[0], m.triangles[t].AB[1], m.triangles[t].AB[2]};
            T.AC = {m.triangles[t].AC[0], m.triangles[t].AC[1], m.triangles[t].AC[2]};
            T.N = {m.triangles[t].ABcrossAC[0], m.triangles[t].ABcrossAC[1], m.triangles[t].ABcrossAC[2]};
            M.t.push_back(T);
            for (V p : {T.A, T.A + T.AB, T.A + T.AC}) {
                M.lo = {fmin(M.lo.x, p.x), fmin(M.lo.y, p.y), fmin(M.lo.z, p.z)};
                M.hi = {fmax(M.hi.x, p.x), fmax(M.hi.y, p.y), fmax(M.hi.z, p.z)};
            }
        }
        M.size = length(M.hi - M.lo);
#if !FRAY_CAMTILE_SCALE
        // The second build: evaluated in FP64 the certificate's only numeric slack that the three scales leave is the record's own rounding -- gatecert_make rounds the
        // half extents UP to the next float and adds the centre's rounding, half a float ulp at least (3e-5 on a wall), 10^8 times what FP64 loses -- and nothing
        // could contradict.  So this build takes that away too: centre and half extents rounded to nearest, the half extents then down.
        for (int k = 0; k < 3; k++) {
            const double lo = (&M.lo.x)[k], hi = (&M.hi.x)[k], c = 0.5 * (lo + hi), half = fmax(hi - c, c - lo);
            M.rec.cf[k] = (float)c;
            float h = (float)half;
            if ((double)h > half) h = nextafterf(h, 0.0f);
            M.rec.hf[k] = h;
        }
#endif
        out.push_back(M);
    }
    printf("%s: %d records\n", path, B.F.nCamSkip);
    delete hs;
    return 0;
}

// ---- the table's origin ---------------------------------------------------------------------------------------------------------------------------------
static int origin_check()
{
    static const int cases[][4] = {{64, 64, 0, 1}, {64, 64, 1, 3}, {64, 64, 2, 3}, {50, 44, 0, 1}, {50, 44, 1, 3}, {50, 44, 2, 3}, {200, 120, 0, 1}, {200, 120, 1, 3}, {200, 120, 2, 3},
                                   {1920, 1080, 0, 1}, {1920, 1080, 3, 8}};
    long items = 0, liveItems = 0;
    for (const auto& c : cases) {
        DFrame F;
        memset(&F, 0, sizeof F);
        F.W = c[0]; F.H = c[1]; F.BW = (F.W + 47) / 48; F.BH = (F.H + 47) / 48;
        F.bucketFirst = c[2]; F.bucketStride = c[3];
        F.nBuckets = frayhip_bucket_count(F.W, F.H, F.bucketFirst, F.bucketStride);
        if (F.nBuckets < 0) { printf("FAIL %dx%d (%d,%d): a bad share\n", c[0], c[1], c[2], c[3]); return 1; }      // (0: a share without a bucket has an empty table)
        const int nItems = F.nBuckets * 2304;
        std::vector<unsigned char> seen((size_t)F.W * F.H, 0);
        for (int t = 0; t < nItems / 64; t++) {
            // what k_cam_tiles stores
            int x0, y0;
            frame_item_pixel(F, t * 64, x0, y0);
            DCamTile e;
            e.skip = 0; e.x0 = (uint16_t)x0; e.y0 = (uint16_t)y0;
            if (e.x0 != x0 || e.y0 != y0 || x0 + 8 > FRAY_CAMTILE_MAX_COORD || y0 + 8 > FRAY_CAMTILE_MAX_COORD) { printf("FAIL %dx%d tile %d: the origin does not fit\n", c[0], c[1], t); return 1; }
            // ... against the bucket numbering of the C ABI
            int bx, by;
            const int bucket = F.bucketFirst + (t / 36) * F.bucketStride;
            if (frayhip_bucket_xy(F.W, F.H, bucket, &bx, &by) || x0 != bx * 48 + (t % 36 % 6) * 8 || y0 != by * 48 + (t % 36 / 6) * 8) { printf("FAIL %dx%d tile %d: not the bucket's tile\n", c[0], c[1], t); return 1; }
            for (int lane = 0; lane < 64; lane++) {
                // what the first bounce takes from the entry, against item_pixel of the lane's item
                const int px = (int)e.x0 + (lane & 7), py = (int)e.y0 + (lane >> 3);
                const bool live = px < F.W && py < F.H;
                int x, y;
                const bool want = frame_item_pixel(F, t * 64 + lane, x, y);
                if (x != px || y != py || want != live) { printf("FAIL %dx%d (%d,%d) item %d: (%d, %d, %d) against item_pixel's (%d, %d, %d)\n", c[0], c[1], c[2], c[3], t * 64 + lane, px, py, (int)live, x, y, (int)want); return 1; }
                items++;
                if (live) { liveItems++; if (seen[(size_t)py * F.W + px]++) { printf("FAIL %dx%d: pixel (%d, %d) twice\n", c[0], c[1], px, py); return 1; } }
            }
        }
        printf("origin %dx%d first %d stride %d: %d tiles\n", c[0], c[1], c[2], c[3], nItems / 64);
    }
    printf("items %ld, in the frame %ld\nOK\n", items, liveItems);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "--origin")) return origin_check();
    if (argc < 3) { fprintf(stderr, "usage: camtile_check N SCENE.fray ... | camtile_check --origin\n"); return 2; }
    const long N = atol(argv[1]);
    std::vector<Mesh> meshes;
    for (int a = 2; a < argc; a++) if (const int rc = load(argv[a], meshes)) return rc;
    if (meshes.empty()) { fprintf(stderr, "no record at all\n"); return 1; }
    const int nClasses = 7;
    long pairs[nClasses] = {0}, cert[nClasses] = {0}, refused[nClasses] = {0}, bad[nClasses] = {0}, rays = 0, hitsSeen = 0, raggedCert = 0, askedPairs = 0, askedRays = 0;
    for (long it = 0; it < N; it++) {
        const int cls = pick(nClasses);
        // the scene of this tile: a mesh and the others of its file (consecutive entries with the same file name stand for one room)
        const int mi = pick((int)meshes.size());
        const Mesh& M = meshes[mi];
        const Tri& T = M.t[pick((int)M.t.size())];
        const V n = normalized(T.N), centre = (M.lo + M.hi) * 0.5;
        const double size = M.size;
        auto inTri = [&](double u, double v) { return T.A + T.AB * u + T.AC * v; };
        auto outline = [&]() {          // a point on the triangle's outline: a corner one time in three
            const int e = pick(3);
            const double w = pick(3) == 0 ? (double)pick(2) : u01();
            return e == 0 ? inTri(w, 0) : e == 1 ? inTri(0, w) : inTri(w, 1 - w);
        };
        int W = 8 * (1 + pick(300)), H = 8 * (1 + pick(200));
        if (cls == 6) { W = 9 + pick(2000); H = 9 + pick(1200); if (W % 8 == 0) W++; if (H % 8 == 0) H++; }
        const double fov = 10 + 110 * u01(), aspect = pick(2) ? (double)W / H : 0.5 + 2 * u01();
        DCamera C = camera(360 * u01(), 180 * u01() - 90, pick(2) ? 0.0 : 360 * u01(), fov, aspect, W, H);
        int x0 = 8 * pick((W + 7) / 8), y0 = 8 * pick((H + 7) / 8);
        if (cls == 6) { if (pick(2)) x0 = (W - 1) / 8 * 8; if (pick(2) || x0 != (W - 1) / 8 * 8) y0 = (H - 1) / 8 * 8; }
        V pos = centre + V{sym(), sym(), sym()} * (size * mag(-1, 1));
        if (cls == 0 || cls == 6) {
            // inside or outside the room: about the mesh, or somewhere in a room of the mesh's scale; looking anywhere or at the mesh
            if (pick(2)) { const V target = centre + V{sym(), sym(), sym()} * (size * 0.8); C = camera_along(target - pos, fov, aspect, W, H); }
        } else if (cls == 1) {
            // a corner ray through (nearly) an edge or a corner of the mesh
            const int c = pick(4);
            const V q = raw_dir(C, x0 + ((c & 1) ? 8 : 0), y0 + ((c & 2) ? 8 : 0));
            const int ok = pick(3);
            const double off = ok == 0 ? mag(-9, -4) : ok == 1 ? size * mag(-16, -9) : size * mag(-4, -1);
            pos = outline() + unit() * off - normalized(q) * (size * mag(-1, 1));
        } else if (cls == 2) {
            // a ray inside the rectangle through the outline, or up to three tile widths beside it
            const double dist = size * mag(-1, 1);
            const V q = normalized(raw_dir(C, x0 + 8 * u01(), y0 + 8 * u01()));
            const double tileWidth = length(normalized(raw_dir(C, x0 + 8, y0 + 8)) - normalized(raw_dir(C, x0, y0))) * dist;
            pos = outline() + unit() * (pick(2) ? 0.0 : tileWidth * 3 * u01()) - q * dist;
        } else if (cls == 3) {
            const int hk = pick(3);
            pos = inTri(u01() * 3 - 1, u01() * 3 - 1) + n * (hk == 0 ? 0.0 : hk == 1 ? sgn() * mag(-9, -5) : sgn() * size * mag(-16, -10));
            if (pick(2)) C = camera_along(pick(2) ? T.AB * sym() + T.AC * sym() + n * (sym() * 0.3) : unit(), fov, aspect, W, H);
        } else if (cls == 4) {
            pos = {M.lo.x + (M.hi.x - M.lo.x) * u01(), M.lo.y + (M.hi.y - M.lo.y) * u01(), M.lo.z + (M.hi.z - M.lo.z) * u01()};
        } else if (cls == 5) {
            // the tile at the image's centre looks along the face; narrow tiles
            W = 8 * (100 + pick(900)); H = 8 * (60 + pick(500));
            const V t = normalized(T.AB * sym() + T.AC * sym());
            x0 = W / 2 / 8 * 8 + 8 * (pick(5) - 2); y0 = H / 2 / 8 * 8 + 8 * (pick(5) - 2);
            if (pick(2)) {
                // slopes against the plane around the record's guard, anywhere beside, above or in the plane
                const double eps = sgn() * (double)M.rec.guard * mag(-1.5, 2.5);
                C = camera_along(t + n * eps, 10 + 20 * u01(), (double)W / H, W, H);
                pos = inTri(u01() * 3 - 1, u01() * 3 - 1) + n * (sgn() * size * mag(-3, 0)) - t * (size * mag(-1, 0.5));
            } else {
                // slopes from 1e-12 to 1e-5, far below the guard, in a view a thousandth of a degree wide: the line crosses the plane just beside the outline,
                // where the triangle test divides by almost nothing
                const double eps = sgn() * mag(-12, -5);
                const V front = t + n * eps;
                C = camera_along(front, mag(-4, 0), (double)W / H, W, H);
                pos = outline() + unit() * (size * mag(-8, -3)) - normalized(front) * (size * mag(-1, 0.5));
            }
        }
        set_pos(C, pos);
        const CamTileView view = cam_tile_view(C);
        const CamTileRays R = cam_tile_rays(view, x0, y0);
        // every record of the mesh's room
        int first = mi, last = mi;
        const std::string room = M.name.substr(0, M.name.find(" node "));
        while (first > 0 && meshes[first - 1].name.compare(0, room.size() + 6, room + " node ") == 0) first--;
        while (last + 1 < (int)meshes.size() && meshes[last + 1].name.compare(0, room.size() + 6, room + " node ") == 0) last++;
        for (int k = first; k <= last; k++) {
            // (the class speaks about the chosen mesh; the room's other meshes are looked at one time in four, so that they do not fill the counts)
            if (k != mi && pick(4)) continue;
            const Mesh& K = meshes[k];
            pairs[cls]++;
            if (!tile_surely_misses_box(K.rec, view, R)) { refused[cls]++; continue; }
            // the box part holds for the tile.  With the tile's guard the pair is certified: every ray counts.  Without it the node is ASKED (dev_camtile.hpp): a ray
            // counts when it passes the per-ray form's guard and bounds in FP32, as dev_trace.hpp camera_guard_nodes evaluates them
            const bool asked = !tile_surely_guarded(K.rec, R);
            if (asked) { refused[cls]++; askedPairs++; } else cert[cls]++;
            bool ragged = false;
            for (int r = 0; r < 24; r++) {
                int lx, ly;
                float jx, jy;
                if (r < 4) { lx = (r & 1) ? 7 : 0; ly = (r & 2) ? 7 : 0; jx = (r & 1) ? 0x1.fffffep-1f : 0.0f; jy = (r & 2) ? 0x1.fffffep-1f : 0.0f; }      // the rectangle's corners
                else {
                    lx = pick(8); ly = pick(8);
                    const int jk = pick(4);
                    jx = jk == 0 ? 0.0f : jk == 1 ? 0x1.fffffep-1f : (float)u01();
                    const int jl = pick(4);
                    jy = jl == 0 ? 0.0f : jl == 1 ? 0x1.fffffep-1f : (float)u01();
                }
                int px = x0 + lx, py = y0 + ly;
                if (px >= W) { px = W - 1; ragged = true; }              // (a pixel outside the frame has no ray: the frame's last column instead)
                if (py >= H) { py = H - 1; ragged = true; }
                const double fx = (double)((float)px + jx), fy = (double)((float)py + jy);
                V o, d;
                screen_ray(C, fx, fy, o, d);
                if (asked) {
                    const float dx = (float)d.x, dy = (float)d.y, dz = (float)d.z, ox = (float)o.x, oy = (float)o.y, oz = (float)o.z;
                    const float dsum = fabsf(dx) + fabsf(dy) + fabsf(dz);
                    if (!(gate_guard_f32(K.rec, dx, dy, dz, dsum) & gate_ray_range(dsum, fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz)), ox + oy + oz))) continue;
                    askedRays++;
                }
                rays++;
                const bool hr = ref_hit(K, o, d), hc = contracted_hit(K, o, d);
                if (hr || hc) {
                    if (bad[cls] < 3) fprintf(stderr, "CONTRADICTION (class %d, %s, %s): a certified tile has a ray a triangle accepts\n  pos %.17g %.17g %.17g  d %.17g %.17g %.17g  tile %d %d of %d x %d, pixel %d %d jitter %.9g %.9g\n",
                                              cls, K.name.c_str(), hr ? "reference" : "contracted copy", o.x, o.y, o.z, d.x, d.y, d.z, x0, y0, W, H, px, py, (double)jx, (double)jy);
                    bad[cls]++;
                    break;
                }
            }
            if (ragged && !asked) raggedCert++;
        }
        // (how often the rays of a refused or certified tile hit the chosen mesh at all: the run is not about empty space)
        { V o, d; screen_ray(C, x0 + 4.0, y0 + 4.0, o, d); if (ref_hit(M, o, d)) hitsSeen++; }
    }
    long totalBad = 0, totalCert = 0;
    bool vacuous = false;
    printf("class: pairs certified refused contradictions\n");
    for (int c = 0; c < nClasses; c++) {
        printf("class %d: %ld %ld %ld %ld\n", c, pairs[c], cert[c], refused[c], bad[c]);
        totalBad += bad[c]; totalCert += cert[c];
        vacuous = vacuous || cert[c] == 0 || refused[c] == 0;
    }
    printf("meshes %zu, tiles %ld, rays %ld, tile centres that hit the chosen mesh %ld, certified pairs of ragged tiles %ld\n", meshes.size(), N, rays, hitsSeen, raggedCert);
    printf("asked pairs (the box part by the tile, the guard left to the rays) %ld, their rays that passed the per-ray guard %ld\n", askedPairs, askedRays);
    printf("certified %ld, contradictions %ld\n", totalCert, totalBad);
    if (vacuous) fprintf(stderr, "a vacuous run: a class without a certified or without a refused pair\n");
    if (FRAY_CAMTILE_SCALE && (askedPairs == 0 || askedRays == 0)) { fprintf(stderr, "a vacuous run: no asked pair, or none of their rays passed the guard\n"); vacuous = true; }
    if (hitsSeen == 0 || raggedCert == 0) { fprintf(stderr, "a vacuous run: no tile looks at its mesh, or no ragged tile was certified\n"); vacuous = true; }
    return (totalBad || vacuous) ? 1 : 0;
}
