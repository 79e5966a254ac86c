// Test harness (CPU only) of tests/test_shade_shortcuts_host.py: the shade shortcuts of frayhip_scene_shade_shortcuts -- finalize_hit, light_nth_sample
// (fray_amd/csrc/dev_shade.hpp) and light_intersect (dev_trace.hpp) -- in their general and their shortcut form side by side, compiled for the host as one lane of a
// wave over the stand-in <hip/hip_runtime.h> of tests/native/hostlane, and the eligibility flags and the world-normal table of scene_arena.hpp fill_editable.
// usage: shade_shortcut_check CORNELL.fray N [--update ORIGINAL.fray EDITED.fray]
// Every output of the two forms is compared by bit pattern:
//   mode 0  N random rays from inside the room: closest_hit's winner through finalize_hit, the ray through light_intersect, the hit point through light_nth_sample;
//   mode 1  adversarial operands on synthetic hit records and rays: components that are +0, -0, subnormal, 2^-500, 2^500, alone and together, in origin and
//           direction; t = 0, t that brings a component of the hit point to an exact zero (hits on x = 0, the left wall's plane); axis-parallel rays;
//   mode 2  light_nth_sample and light_intersect on shade points and rays in, above and below the light's plane, on the cornell light, on a light mirrored in x
//           (negative diagonal entries) and -- only in the build with -DFRAY_LIGHT_ZERO_OFFSET_OK=1 -- on a mirrored light whose offset has a -0 component.
// A case whose general form has a non-finite direction or local hit point lies outside the proofs' precondition (finite operands) and is counted, not compared.
// light_intersect: the answers must agree, and `dist` by bits unless neither passes closest_hit's dist < 1e99.  light_nth_sample: samplePos and the generator's state by
// bits; `color` by bits unless the shade point lies exactly in the light's plane (sp.y a zero), where the sign of its zero may differ: counted.
// Then the eligibility of edited lights (a zero offset component, an off-diagonal entry, xSubd 3), the table against finalize_hit's general form for every triangle,
// a triangle whose normal has a -0 component, and with --update the flags and the table across arena_update.
// Prints the counts; exit code 1 with contradictions or a FAIL line.
#include <hip/hip_runtime.h>      // the stand-in of tests/native/hostlane

#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "dev_shade.hpp"
#include "host_scene.h"
#include "scene_arena.hpp"

lanes_t lanes(bool p) { return p ? 1ull : 0ull; }
bool lane_of(lanes_t m) { return (m & 1ull) != 0; }

using frayhip_arena::ArenaBuilt;

// `zeros`: that many first draws are the word 0 (a sample on the edge of its cell: cell 2 of 4 then starts at the light's centre line, pl.x an exact zero)
struct Gen {
    uint64_t s; int zeros;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; if (zeros > 0) { zeros--; return 0u; } return (uint32_t)(s >> 32); }
};
static double uni(Gen& g) { return (g.next() + 0.5) / 4294967296.0; }

static uint64_t bitsOf(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static bool same(double a, double b) { return bitsOf(a) == bitsOf(b); }
static bool same3(V3 a, V3 b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }
static bool finite3(V3 v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }
static bool sameC(C3 a, C3 b) { return !memcmp(&a, &b, sizeof a); }

// an arena with every table in a heap block of its own, placed
struct Placed {
    ArenaBuilt B;
    std::vector<std::vector<unsigned char>> blocks;
    DScene S;
    void place()
    {
        blocks.resize(B.tables.size());
        std::vector<unsigned char*> w(B.tables.size());
        for (size_t t = 0; t < B.tables.size(); t++) {
            blocks[t].assign(B.host.begin() + B.tables[t].off, B.host.begin() + B.tables[t].off + B.tables[t].bytes);
            if (blocks[t].empty()) blocks[t].resize(1);
            w[t] = blocks[t].data();
        }
        memset(&S, 0, sizeof S);
        frayhip_arena::arena_place(B.F, B.meshTables.data(), B.texelOffset.data(), w.data(), w.data(), S);
        S.maxTraceDepth = 6; S.gi = 1;
    }
};

static long long nCases[3], nBad[3], nOutside[3], nPlaneColor, nPlaneColorDiffers, nLightHits, nMeshHits;
static int shown;
static void bad(int mode, const char* what, V3 o, V3 d)
{
    nBad[mode]++;
    if (shown++ < 12) printf("contradiction (mode %d) %s: o = (%a, %a, %a) d = (%a, %a, %a)\n", mode, what, o.x, o.y, o.z, d.x, d.y, d.z);
}

// finalize_hit's two forms on one hit record
static void check_finalize(int mode, const DScene& S, const HitRec& h, V3 o, V3 d)
{
    nCases[mode]++;
    const DNode& N = S.nodes[h.node];
    const V3 ldir = normalized(mulM(d, N.T.inv)), ipl = mulM(o - ld3(N.T.off), N.T.inv) + ldir * h.t;
    if (!(finite3(o) && finite3(ldir) && finite3(ipl) && std::isfinite(h.t))) { nOutside[mode]++; return; }
    HitInfo a, b;
    memset(&a, 0xA5, sizeof a); memset(&b, 0x5A, sizeof b);
    finalize_hit<0, false, false, false>(S, h, o, d, false, a);
    finalize_hit<0, false, false, true>(S, h, o, d, false, b);
    if (!same3(a.ip, b.ip)) bad(mode, "finalize_hit ip", o, d);
    if (!same3(a.norm, b.norm)) bad(mode, "finalize_hit norm", o, d);
    if (!same3(a.dNdx, b.dNdx) || !same3(a.dNdy, b.dNdy) || !same(a.u, b.u) || !same(a.v, b.v)) bad(mode, "finalize_hit dNdx / dNdy / uv", o, d);
}

static void check_light_intersect(int mode, const DLight& L, V3 o, V3 d)
{
    nCases[mode]++;
    const V3 ldir = normalized(mulM(d, L.T.inv));
    if (!(finite3(o) && finite3(d) && finite3(ldir))) { nOutside[mode]++; return; }
    Cnt c;
    memset(&c, 0, sizeof c);
    double da = -1, db = -1;
    const bool ha = light_intersect<0, false>(L, o, d, da, c, false), hb = light_intersect<0, true>(L, o, d, db, c, true);
    if (ha != hb) { bad(mode, "light_intersect's answer", o, d); return; }
    if (ha) nLightHits++;
    if (ha && !same(da, db) && (da < 1e99 || db < 1e99)) bad(mode, "light_intersect dist", o, d);
}

static void check_light_sample(int mode, const DLight& L, int idx, V3 x, uint64_t seed, int zeros = 0)
{
    nCases[mode]++;
    if (!finite3(x)) { nOutside[mode]++; return; }
    Gen ga{seed, zeros}, gb{seed, zeros};
    V3 pa, pb;
    C3 ca, cb;
    light_nth_sample<false>(L, idx, x, ga, pa, ca, false);
    light_nth_sample<true>(L, idx, x, gb, pb, cb, true, true);
    if (!same3(pa, pb)) bad(mode, "light_nth_sample samplePos", x, pa);
    if (ga.s != gb.s || ga.zeros != gb.zeros) bad(mode, "light_nth_sample's draws", x, pa);
    const V3 sp = mulM(x - ld3(L.T.off), L.T.inv);
    if (sp.y == 0) { nPlaneColor++; if (!sameC(ca, cb)) nPlaneColorDiffers++; }
    else if (!sameC(ca, cb)) bad(mode, "light_nth_sample color", x, pa);
}

static const double SPECIAL[] = {0.0, -0.0, 4.9406564584124654e-324, -4.9406564584124654e-324, 0x1p-500, -0x1p-500, 0x1p500, -0x1p500, 1.0, -1.0};
static double pick(Gen& g, double scale)
{
    const uint32_t k = g.next() % 16;
    return k < 10 ? SPECIAL[k] : (2 * uni(g) - 1) * scale;
}

static int fail(const char* what) { printf("FAIL %s\n", what); return 1; }

static DLight dlight_of(const frayhip_light& l)
{
    DLight o;
    memset(&o, 0, sizeof o);
    o.kind = l.kind; o.xSubd = l.xSubd; o.ySubd = l.ySubd;
    o.xShift = -1;
    if ((l.xSubd & (l.xSubd - 1)) == 0) for (o.xShift = 0; (1 << o.xShift) < l.xSubd;) o.xShift++;
    memcpy(o.color, l.color, sizeof o.color); o.power = l.power;
    frayhip_arena::detail::putX(o.T, l.T);
    memcpy(o.center, l.center, sizeof o.center);
    o.area = l.area; o.areaXsize = 1.0 / l.xSubd; o.areaYsize = 1.0 / l.ySubd;
    return o;
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: shade_shortcut_check CORNELL.fray N [--update ORIGINAL.fray EDITED.fray]\n"); return 2; }
    std::string err;
    frayhost::HostScene* hs = frayhost::parse_scene_file(argv[1], err);
    if (!hs) { fprintf(stderr, "%s: %s\n", argv[1], err.c_str()); return 2; }
    const long long N = atoll(argv[2]);
    const frayhip_scene_desc& d = hs->desc;
    Placed P;
    frayhip_arena::arena_build(d, P.B);
    P.place();
    const DScene& S = P.S;
    printf("flags: shadeIdentity %d lightsDiagonal %d normStride %d nodes %d lights %d xShift %d\n", S.shadeIdentity, S.lightsDiagonal, S.normStride, S.nNodes, S.nLights,
           S.nLights ? S.lights[0].xShift : -9);
    if (!S.shadeIdentity || !S.lightsDiagonal || S.nLights != 1 || S.lights[0].xShift != 2) return fail("the scene is not eligible: cornell_box.fray is expected");
    const DLight& L = S.lights[0];

    // the table against the general form's normal, every triangle of every node
    int nTri = 0;
    for (int i = 0; i < S.nNodes; i++)
        for (int t = 0; t < S.nodes[i].tlTris; t++, nTri++) {
            HitRec h{i, t, 1.0, 1.0, 0, 0};
            HitInfo a;
            finalize_hit<0>(S, h, v3(1, 2, 3), v3(0, 0, 1), false, a);
            if (!same3(a.norm, ld3(S.worldNormals + 3 * (i * S.normStride + t)))) return fail("a table entry is not the general form's normal");
        }
    {   // a normal with a -0 component through the identity: (+0) * 1 + ... keeps no -0 unless every term is -0
        const double g[3] = {-0.0, 0.6, -0.8}, I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        double w[3];
        frayhip_arena::detail::world_normal(g, I9, w);
        const V3 e = normalized(mulM(v3(g[0], g[1], g[2]), I9));
        if (!same3(e, v3(w[0], w[1], w[2])) || !same(w[0], 0.0)) return fail("world_normal of a normal with a -0 component");
    }
    printf("table: %d entries equal the general form's normals\n", nTri);

    Gen g{20261020, 0};
    // ---- mode 0 ----
    for (long long k = 0; k < N; k++) {
        const V3 o = v3(20 + 510 * uni(g), 20 + 500 * uni(g), 20 + 520 * uni(g));
        V3 dir;
        do dir = v3(2 * uni(g) - 1, 2 * uni(g) - 1, 2 * uni(g) - 1); while (lengthSqr(dir) > 1 || lengthSqr(dir) < 1e-4);
        dir = normalized(dir);
        Cnt c;
        memset(&c, 0, sizeof c);
        HitRec h;
        closest_hit<0>(S, o, dir, h, c);
        check_light_intersect(0, L, o, dir);
        if (h.node < 0) continue;
        nMeshHits++;
        check_finalize(0, S, h, o, dir);
        HitInfo info;
        finalize_hit<0>(S, h, o, dir, false, info);
        check_light_sample(0, L, (int)(g.next() % 16), info.ip, g.next());
    }
    // ---- mode 1 ----
    const long long N1 = N / 2 + 1000;
    for (long long k = 0; k < N1; k++) {
        V3 o = v3(pick(g, 550), pick(g, 550), pick(g, 550)), dir = v3(pick(g, 1), pick(g, 1), pick(g, 1));
        const int node = (int)(g.next() % S.nNodes), tri = (int)(g.next() % S.nodes[node].tlTris);
        double t = uni(g) * 800;
        switch (g.next() % 6) {
            case 0: t = 0; break;
            case 1: t = 4.9406564584124654e-324; break;
            case 2: o.x = 100 + (g.next() % 400); dir = v3(-1, pick(g, 1) * 0, pick(g, 1) * 0); t = o.x; break;          // onto x = 0 along the axis: ipl.x is an exact zero
            case 3: o.y = 0.5 * (g.next() % 900); dir = v3(0.0 * pick(g, 1), -1, -0.0); t = o.y; break;
            case 4: { const V3 u = normalized(v3(-3, 4 * (uni(g) - 0.5), 0)); o.x = -u.x * 64; t = 64; dir = u; break; }      // o.x + ldir.x * t may cancel to a zero
            default: break;
        }
        check_finalize(1, S, HitRec{node, tri, t, t, 0, 0}, o, dir);
        check_light_intersect(1, L, o, dir);
        check_light_sample(1, L, (int)(g.next() % 16), o, g.next());
    }
    // ---- mode 2 ----
    std::vector<DLight> lights{L};
    {
        frayhip_light m = d.lights[0];
        m.T.m[0] = -m.T.m[0]; m.T.invM[0] = -m.T.invM[0];
        m.T.m[8] = -m.T.m[8]; m.T.invM[8] = -m.T.invM[8];
        if (!frayhip_arena::detail::light_is_diagonal(m)) return fail("a mirrored light reads ineligible");
        lights.push_back(dlight_of(m));
        m.T.offset[0] = -0.0; m.T.offset[2] = -0.0;
        const bool through = frayhip_arena::detail::light_is_diagonal(m);
        printf("a mirrored light with a -0 offset component: %s\n", through ? "ELIGIBLE (the rule is switched off in this build)" : "not eligible");
        if (through != (FRAY_LIGHT_ZERO_OFFSET_OK != 0)) return fail("the zero-offset rule");
        if (through) lights.push_back(dlight_of(m));
    }
    const long long N2 = N / 4 + 1000;
    for (const DLight& Lk : lights)
        for (long long k = 0; k < N2; k++) {
            const V3 off = ld3(Lk.T.off);
            // shade points in the light's plane, on its axes, at its centre; rays from such points, along the axes and random
            V3 x = v3(off.x + pick(g, 200), off.y + (g.next() % 3 == 0 ? 0.0 : -uni(g) * 500), off.z + pick(g, 200));
            if (g.next() % 4 == 0) x.x = off.x == 0 ? pick(g, 1) * 0 : off.x;
            if (g.next() % 4 == 0) x.z = off.z == 0 ? pick(g, 1) * 0 : off.z;
            for (int idx = 0; idx < 16; idx += 5) check_light_sample(2, Lk, idx, x, g.next(), (int)(g.next() % 3));
            V3 dir = v3(pick(g, 1), uni(g), pick(g, 1));
            if (g.next() % 3 == 0) dir = v3(pick(g, 1) * 0, 1, pick(g, 1) * 0);
            x.y = off.y - uni(g) * 500;
            check_light_intersect(2, Lk, x, dir);
        }

    // ---- eligibility of edited lights ----
    {
        frayhip_light l = d.lights[0];
        if (!frayhip_arena::detail::light_is_diagonal(l)) return fail("cornell's light reads ineligible");
        frayhip_light z = l; z.T.offset[1] = 0.0;
        frayhip_light od = l; od.T.m[1] = 0.25;
        frayhip_light oi = l; oi.T.invM[5] = -1e-300;
        frayhip_light pt = l; pt.kind = FRAYHIP_LIGHT_POINT;
        frayhip_light nf = l; nf.T.offset[2] = INFINITY;
        if (!FRAY_LIGHT_ZERO_OFFSET_OK && frayhip_arena::detail::light_is_diagonal(z)) return fail("a light with a zero offset component reads eligible");
        if (frayhip_arena::detail::light_is_diagonal(od) || frayhip_arena::detail::light_is_diagonal(oi)) return fail("a light with an off-diagonal entry reads eligible");
        if (frayhip_arena::detail::light_is_diagonal(pt) || frayhip_arena::detail::light_is_diagonal(nf)) return fail("a point light or a non-finite offset reads eligible");
        // through arena_build: xSubd 3 takes the division (no shift), the other edits clear the flag
        std::vector<frayhip_light> ls(d.lights, d.lights + d.n_lights);
        frayhip_scene_desc e = d;
        e.lights = ls.data();
        ArenaBuilt E;
        ls[0].xSubd = 3;
        frayhip_arena::arena_build(e, E);
        const DLight* EL = (const DLight*)(E.host.data() + E.tables[E.F.tLights].off);
        if (EL[0].xShift != -1 || !E.F.lightsDiagonal) return fail("xSubd 3: a shift, or the flag cleared");
        for (int s = 1; s <= 64; s++) {
            ls[0].xSubd = s;
            frayhip_arena::arena_build(e, E);
            EL = (const DLight*)(E.host.data() + E.tables[E.F.tLights].off);
            const bool pow2 = (s & (s - 1)) == 0;
            if (pow2 != (EL[0].xShift >= 0) || (pow2 && (1 << EL[0].xShift) != s)) return fail("xShift is not log2(xSubd) of a power of two, -1 otherwise");
        }
        ls[0] = od;
        frayhip_arena::arena_build(e, E);
        if (E.F.lightsDiagonal || !E.F.shadeIdentity) return fail("an off-diagonal entry through arena_build");
        printf("eligibility: zero offset, off-diagonal entries, point light, non-finite offset, xSubd 1 .. 64 read as they should\n");
    }
    // the cell by mask and shift against the division, every idx of every power-of-two light up to 64 x 3
    for (int sh = 0; sh <= 6; sh++)
        for (int idx = 0; idx < (1 << sh) * 3; idx++)
            if ((idx & ((1 << sh) - 1)) != idx % (1 << sh) || (idx >> sh) != idx / (1 << sh)) return fail("mask and shift against % and /");

    // ---- the flags and the table across arena_update ----
    if (argc >= 6 && !strcmp(argv[3], "--update")) {
        frayhost::HostScene* ho = frayhost::parse_scene_file(argv[4], err);
        frayhost::HostScene* he = ho ? frayhost::parse_scene_file(argv[5], err) : nullptr;
        if (!ho || !he) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
        ArenaBuilt O, E, U;
        frayhip_arena::arena_build(ho->desc, O);
        frayhip_arena::arena_build(he->desc, E);
        frayhip_arena::arena_build(ho->desc, U);
        frayhip_arena::arena_update(he->desc, U);
        printf("updated: shadeIdentity %d -> %d, lightsDiagonal %d -> %d\n", O.F.shadeIdentity, U.F.shadeIdentity, O.F.lightsDiagonal, U.F.lightsDiagonal);
        if (U.F.shadeIdentity != E.F.shadeIdentity || U.F.lightsDiagonal != E.F.lightsDiagonal) return fail("the updated flags are not the fresh arena's");
        if (U.host.size() != E.host.size() || memcmp(U.host.data(), E.host.data(), E.host.size())) return fail("the updated arena is not the fresh one");
        frayhip_arena::arena_update(ho->desc, U);
        printf("updated back: shadeIdentity %d, lightsDiagonal %d\n", U.F.shadeIdentity, U.F.lightsDiagonal);
        if (U.F.shadeIdentity != O.F.shadeIdentity || U.F.lightsDiagonal != O.F.lightsDiagonal) return fail("the flags updated back are not the original's");
        if (memcmp(U.host.data(), O.host.data(), O.host.size())) return fail("the arena updated back is not the original");
        const ArenaBuilt& T = U;
        if (T.tables[T.F.tWorldNormals].bytes != (size_t)ho->desc.n_nodes * T.F.normStride * 24 || T.F.tWorldNormals != (int)T.tables.size() - 1)
            return fail("the table's size or place");
        delete ho; delete he;
    }

    long long cases = 0, contradictions = 0;
    for (int m = 0; m < 3; m++) { cases += nCases[m]; contradictions += nBad[m]; }
    printf("cases per mode: %lld %lld %lld\n", nCases[0], nCases[1], nCases[2]);
    printf("outside the precondition per mode: %lld %lld %lld\n", nOutside[0], nOutside[1], nOutside[2]);
    printf("contradictions per mode: %lld %lld %lld\n", nBad[0], nBad[1], nBad[2]);
    printf("mesh hits %lld, light hits %lld; shade points in the light's plane %lld, their colour's zero differs in sign %lld\n", nMeshHits, nLightHits, nPlaneColor, nPlaneColorDiffers);
    printf("cases %lld, contradictions %lld\n", cases, contradictions);
    delete hs;
    return contradictions ? 1 : 0;
}
