// The scene arena on the host: every read-only table the kernels follow, made from a frayhip_scene_desc in two steps that need no device.
//
//   arena_build   description -> the arena's bytes with every inner pointer still null, the list of its tables (one per block, in the
//                 order they were laid out) and the scene facts that choose kernels (ArenaFacts);
//   arena_update  the editable part of an edited description (include/frayhip.h, frayhip_scene_update) written again into an arena built earlier: the
//                 tables whose size no mesh and no texel decides, by the very code arena_build filled them with, and the facts that follow;
//   arena_place   given, for every table, where it can be written now and where it will live, writes the inner pointers (a mesh's arrays,
//                 a tree-less node's triangles, a texture's texels) and fills the DScene.
//
// frayhip_scene_create (capi.hip) places all tables at `device base + offset` and uploads the bytes as one allocation.  The host harness of
// tests/native/hostlane places each table in a heap block of its own, so that an index past a table's end is an error there and not a read of
// the neighbouring table.  Host code only: nothing here is compiled for the device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

#include "dev_scene.hpp"

namespace frayhip_arena {

struct ArenaTable { uint64_t off, bytes; };

// The tables place() writes to or points at, as indices into ArenaBuilt::tables (two empty tables may share an offset, an index names one).
struct ArenaMeshTables { int32_t tris, attrs, kd, kdBox, refs, ltris, ltris32; };

// Plain data: what a description leaves behind besides the tables themselves.
struct ArenaFacts {
    int32_t extGeometry, kdMeshes, textured, whittedNeedsRecursion, lightDraws, lightSampleCount, specFanMax;
    int32_t nGates, gatesExact, nSegPlanes, nSegNodes, segCertAll;
    int32_t nTightGates;                      // gates whose entry in the table's tight half differs: eligible meshes (dev_gatecert.hpp)
    int32_t nCamSkip, tCamSkip;               // miss records of the first bounce (dev_scene.hpp DCamSkip) and their table
    int32_t shadeIdentity, lightsDiagonal;    // the shade shortcuts' eligibility (dev_scene.hpp DScene::shadeIdentity, lightsDiagonal): of the nodes, of the lights
    int32_t normStride, tWorldNormals;        // the world-normal table (DScene::worldNormals): entries per node (fixed at arena_build), and the table
    int32_t nNodes, nLights, nMeshes, nTextures;
    int32_t envPresent, envLoaded, envWidth[6], envHeight[6];
    int64_t envTexelOffset[6];
    int32_t tNodes, tNodesX, tGates, tSegPlanes, tSegMasks, tPlanes, tSpheres, tCubes, tCsgs, tTexels, tShaders, tLayers, tLights, tMeshes, tTex;
};

struct ArenaBuilt {
    std::vector<unsigned char> host;          // the arena, inner pointers null
    std::vector<ArenaTable> tables;
    std::vector<ArenaMeshTables> meshTables;  // per mesh
    std::vector<int64_t> texelOffset;         // per texture: its first texel in the texel pool (floats)
    ArenaFacts F;
};

namespace detail {

// One allocation holding every read-only table of a scene.
struct Arena {
    std::vector<unsigned char>& host;
    std::vector<ArenaTable>& tables;
    size_t add(const void* p, size_t bytes, size_t align = 256)
    {
        size_t off = (host.size() + align - 1) / align * align;
        host.resize(off + bytes);
        if (bytes) memcpy(host.data() + off, p, bytes);
        tables.push_back(ArenaTable{(uint64_t)off, (uint64_t)bytes});
        return off;
    }
    // an aligned, zero-filled slot that is filled in later
    size_t reserve(size_t bytes)
    {
        size_t off = add(nullptr, 0);
        host.resize(off + bytes);
        tables.back().bytes = bytes;
        return off;
    }
    int32_t last() const { return (int32_t)tables.size() - 1; }
};

inline void put3(double* o, const double* p) { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
inline void putX(DXform& X, const frayhip_transform& T)
{
    put3(X.off, T.offset);
    memcpy(X.m, T.m, sizeof X.m);
    memcpy(X.inv, T.invM, sizeof X.inv);
}

inline bool shader_uses_uv(const frayhip_scene_desc& d, int s, int depth = 0)
{
    if (s < 0 || s >= d.n_shaders || depth > 40) return false;
    const frayhip_shader& sh = d.shaders[s];
    auto texUV = [&](int t) { return t >= 0 && t < d.n_textures && d.textures[t].kind != FRAYHIP_TEX_FRESNEL; };
    if (texUV(sh.texture)) return true;
    if (sh.kind == FRAYHIP_SHADER_LAYERED)
        for (int i = 0; i < sh.layer_count; i++) {
            const frayhip_layer& L = d.layers[sh.layer_begin + i];
            if (texUV(L.texture) || shader_uses_uv(d, L.shader, depth + 1)) return true;
        }
    return false;
}

// Everything of the arena that the EDITABLE part of a description decides (include/frayhip.h, frayhip_scene_update): the node tables with their gates and
// segment planes, the primitives, shaders, layers, lights and texture records, and the scene facts that follow from them.  arena_build runs it on the
// freshly laid out arena and arena_update on an arena built earlier, so an updated arena equals a fresh one byte for byte.  tab[t] is where table t
// can be written.  Read besides `d`: the DMesh table (the header scalars of every mesh) and the DTri table of every mesh without a KD-tree and with
// at most FRAY_GATECERT_MAX_TRIS triangles (arena_keeps_tris: the segment planes of the small ones, the tight gate records of the others, the first bounce's miss records of both) -- never a
// mesh array or the texel pool of `d`.  Every inner pointer is written null
// (arena_place); the unused tails of the gate and segment-plane tables are zeroed.  F: the t* indices and the counts are read, the editable facts written.
// normalized(mulM(g, m)) as finalize_hit (dev_shade.hpp) evaluates it for a flat triangle's normal, operation for operation (dev_math.hpp mulM, length, normalized in
// the exact arithmetic): IEEE multiplications, additions, one square root and one division, which give the same bits whoever performs them.
inline void world_normal(const double* g, const double* m, double* out)
{
    const double x = g[0] * m[0] + g[1] * m[3] + g[2] * m[6], y = g[0] * m[1] + g[1] * m[4] + g[2] * m[7], z = g[0] * m[2] + g[1] * m[5] + g[2] * m[8];
    const double r = 1.0 / std::sqrt(x * x + y * y + z * z);
    out[0] = x * r; out[1] = y * r; out[2] = z * r;
}
// A light the diagonal forms of light_intersect and light_nth_sample may serve (DScene::lightsDiagonal): a RectLight whose m and inv have zero off-diagonal and
// finite diagonal entries and whose offset's components are finite and NONZERO -- the addition of the offset is what erases the sign of a zero product, and a -0
// component would keep it.
#ifndef FRAY_LIGHT_ZERO_OFFSET_OK
#define FRAY_LIGHT_ZERO_OFFSET_OK 0    // tests/native/shade_shortcut_check.cpp builds a second time with 1 to show that it sees what the rule is there for
#endif
inline bool light_is_diagonal(const frayhip_light& l)
{
    bool ok = l.kind == FRAYHIP_LIGHT_RECT;
    for (int k = 0; k < 9; k++) {
        const bool diag = k == 0 || k == 4 || k == 8;
        ok = ok && (diag ? std::isfinite(l.T.m[k]) && std::isfinite(l.T.invM[k]) : l.T.m[k] == 0.0 && l.T.invM[k] == 0.0);
    }
    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(l.T.offset[k]) && (FRAY_LIGHT_ZERO_OFFSET_OK || l.T.offset[k] != 0.0);
    return ok;
}
inline bool arena_keeps_tris(const DMesh& M) { return !M.hasKd && M.nTris > 0 && M.nTris <= FRAY_GATECERT_MAX_TRIS; }
inline void fill_editable(const frayhip_scene_desc& d, const ArenaMeshTables* meshTables, ArenaFacts& F, unsigned char* const* tab)
{
    const DMesh* const meshes = (const DMesh*)tab[F.tMeshes];
    F.extGeometry = F.whittedNeedsRecursion = F.lightDraws = F.lightSampleCount = F.specFanMax = 0;
    for (int i = 0; i < d.n_nodes; i++) {
        int k = d.geoms[d.nodes[i].geom].kind;
        if (k == FRAYHIP_GEOM_CUBE || k == FRAYHIP_GEOM_CSG) F.extGeometry = 1;   // selects the <ST | 2> kernel variants
    }
    std::vector<DNode> nodes(d.n_nodes);
    for (int i = 0; i < d.n_nodes; i++) {
        const frayhip_node& n = d.nodes[i];
        putX(nodes[i].T, n.T);
        nodes[i].geomKind = d.geoms[n.geom].kind;
        nodes[i].geomIndex = d.geoms[n.geom].index;
        nodes[i].shader = n.shader;
        nodes[i].bumpTex = n.bump_tex;
        nodes[i].xfClass = i;
        {
            static const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z3[3] = {0, 0, 0};       // +0.0 everywhere: a -0.0 in the file's transform is not the identity
            nodes[i].xfIdentity = (!memcmp(n.T.offset, Z3, sizeof Z3) && !memcmp(n.T.m, I9, sizeof I9) && !memcmp(n.T.invM, I9, sizeof I9)) ? 1 : 0;
        }
        for (int j = 0; j < i; j++)
            if (!memcmp(d.nodes[j].T.offset, n.T.offset, sizeof n.T.offset) && !memcmp(d.nodes[j].T.invM, n.T.invM, sizeof n.T.invM) &&
                !memcmp(d.nodes[j].T.m, n.T.m, sizeof n.T.m)) {
                nodes[i].xfClass = nodes[j].xfClass;
                break;
            }
        int sk = d.shaders[n.shader].kind;
        if (sk == FRAYHIP_SHADER_REFL || sk == FRAYHIP_SHADER_REFR || sk == FRAYHIP_SHADER_LAYERED) F.whittedNeedsRecursion = 1;
    }
    DPlane* const planes = (DPlane*)tab[F.tPlanes];
    for (int i = 0; i < d.n_planes; i++) { planes[i].limit = d.planes[i].limit; planes[i].height = d.planes[i].height; }
    DSphere* const spheres = (DSphere*)tab[F.tSpheres];
    for (int i = 0; i < d.n_spheres; i++) { put3(spheres[i].O, d.spheres[i].O); spheres[i].R = d.spheres[i].R; }
    DCube* const cubes = (DCube*)tab[F.tCubes];
    for (int i = 0; i < d.n_cubes; i++) { put3(cubes[i].O, d.cubes[i].O); cubes[i].halfSide = d.cubes[i].halfSide; }
    std::vector<DTexture> tex(d.n_textures);
    for (int i = 0; i < d.n_textures; i++) {
        const frayhip_texture& t = d.textures[i];
        DTexture& o = tex[i];
        o.kind = t.kind; o.width = t.width; o.height = t.height; o.pad = 0;
        memcpy(o.color1, t.color1, sizeof o.color1);
        memcpy(o.color2, t.color2, sizeof o.color2);
        o.scaling = t.scaling; o.bumpIntensity = t.bumpIntensity; o.ior = t.ior;
        o.texels = nullptr;   // arena_place
    }
    std::vector<DShader> shaders(d.n_shaders);
    for (int i = 0; i < d.n_shaders; i++) {
        const frayhip_shader& s = d.shaders[i];
        DShader& o = shaders[i];
        o.kind = s.kind; o.texture = s.texture;
        memcpy(o.color, s.color, sizeof o.color);
        memcpy(o.specularColor, s.specularColor, sizeof o.specularColor);
        memcpy(o.mult, s.mult, sizeof o.mult);
        o.numSamples = s.numSamples;
        o.exponent = s.exponent; o.specularMultiplier = s.specularMultiplier; o.glossiness = s.glossiness;
        o.deflectionScaling = s.deflectionScaling; o.ior = s.ior;
        o.layerBegin = s.layer_begin; o.layerCount = s.layer_count;
        o.usesUV = shader_uses_uv(d, i);
        o.pad = 0;
    }
    if (!shaders.empty()) memcpy(tab[F.tShaders], shaders.data(), shaders.size() * sizeof(DShader));
    std::vector<DLayer> layers(d.n_layers);
    for (int i = 0; i < d.n_layers; i++) {
        layers[i].shader = d.layers[i].shader; layers[i].texture = d.layers[i].texture;
        memcpy(layers[i].opacity, d.layers[i].opacity, sizeof layers[i].opacity);
        layers[i].pad = 0;
    }
    if (!layers.empty()) memcpy(tab[F.tLayers], layers.data(), layers.size() * sizeof(DLayer));
    std::vector<DLight> lights(d.n_lights);
    bool anyLightDraws = false;
    for (int i = 0; i < d.n_lights; i++) {
        const frayhip_light& l = d.lights[i];
        DLight& o = lights[i];
        o.kind = l.kind; o.xSubd = l.xSubd; o.ySubd = l.ySubd;
        o.xShift = -1;                                                   // light_nth_sample's cell by mask and shift
        if (l.kind == FRAYHIP_LIGHT_RECT && l.xSubd > 0 && (l.xSubd & (l.xSubd - 1)) == 0)
            for (o.xShift = 0; (1 << o.xShift) < l.xSubd;) o.xShift++;
        memcpy(o.color, l.color, sizeof o.color);
        o.power = l.power;
        put3(o.pos, l.pos);
        putX(o.T, l.T);
        put3(o.center, l.center);
        o.area = l.area;
        F.lightSampleCount += l.kind == FRAYHIP_LIGHT_RECT ? l.xSubd * l.ySubd : 1;
        if (l.kind == FRAYHIP_LIGHT_RECT) F.lightDraws = 1;
        if (l.kind == FRAYHIP_LIGHT_RECT) anyLightDraws = true;          // RectLight::getNthSample draws two words per sample (lights.cpp:62-63)
        o.areaXsize = 1.0 / l.xSubd;
        o.areaYsize = 1.0 / l.ySubd;
    }
    // glossy fans may be drawn ahead (dev_whitted.hpp) where nothing under them is likely to draw: no light that samples, a fan of eight or more
    F.specFanMax = 0;
    if (!anyLightDraws)
        for (int i = 0; i < d.n_shaders; i++)
            if (d.shaders[i].kind == FRAYHIP_SHADER_REFL && d.shaders[i].glossiness != 1.0 && d.shaders[i].numSamples >= 8)
                F.specFanMax = std::max(F.specFanMax, (int)d.shaders[i].numSamples);
    if (!lights.empty()) memcpy(tab[F.tLights], lights.data(), lights.size() * sizeof(DLight));
    std::vector<DNodeX> nodesX(nodes.size());
    for (int i = 0; i < d.n_nodes; i++) {
        DNode& N = nodes[i];
        DNodeX& X = nodesX[i];
        N.tlTris = 0; N.tlCulling = 0; N.tlPtr = nullptr; N.boxMax = 0; N.gated = 0; N.segNode = 0;
        for (int k = 0; k < 3; k++) N.bmin[k] = N.bmax[k] = X.bminE[k] = X.bmaxE[k] = 0;
        if (N.geomKind == FRAYHIP_GEOM_MESH && !meshes[N.geomIndex].hasKd) {
            const DMesh& M = meshes[N.geomIndex];
            N.tlTris = M.nTris; N.tlCulling = M.culling;      // (tlPtr: arena_place)
            put3(N.bmin, M.bmin); put3(N.bmax, M.bmax);
            N.boxMax = M.boxMax;
            for (int k = 0; k < 3; k++) { X.bminE[k] = N.bmin[k] - 1e-6; X.bmaxE[k] = N.bmax[k] + 1e-6; }
        }
    }
    // Bounds of a geometry tree in its own (local) space: every point an intersection of the tree can lie on.  Plus: both operands; Minus: the left one
    // (a ray that has no intersection with the left operand is never inside the difference); And: either operand alone bounds the result, the smaller
    // box is taken.  A Plane operand makes its tree unbounded (ok = false) unless the operator hides it.
    struct GB { bool ok; double lo[3], hi[3]; };
    std::function<GB(int, int)> bounds = [&](int g, int depth) -> GB {
        GB b{true, {0, 0, 0}, {0, 0, 0}};
        if (g < 0 || g >= d.n_geoms || depth > FRAY_CSG_DEPTH + 1) { b.ok = false; return b; }
        const int kind = d.geoms[g].kind, idx = d.geoms[g].index;
        if (kind == FRAYHIP_GEOM_PLANE) {
            // never bounded here: Plane::intersect divides 0 by 0 for a horizontal ray that starts at the plane's height and then reports a hit at NaN
            // (geometry.cpp:35-41: no comparison with NaN is true), wherever the ray is -- no box holds that
            b.ok = false; return b;
        } else if (kind == FRAYHIP_GEOM_SPHERE) {
            for (int k = 0; k < 3; k++) { b.lo[k] = d.spheres[idx].O[k] - std::fabs(d.spheres[idx].R); b.hi[k] = d.spheres[idx].O[k] + std::fabs(d.spheres[idx].R); }
        } else if (kind == FRAYHIP_GEOM_CUBE) {
            for (int k = 0; k < 3; k++) { b.lo[k] = d.cubes[idx].O[k] - std::fabs(d.cubes[idx].halfSide); b.hi[k] = d.cubes[idx].O[k] + std::fabs(d.cubes[idx].halfSide); }
        } else if (kind == FRAYHIP_GEOM_MESH) {
            for (int k = 0; k < 3; k++) { b.lo[k] = meshes[idx].bmin[k]; b.hi[k] = meshes[idx].bmax[k]; }
        } else if (kind == FRAYHIP_GEOM_CSG) {
            const frayhip_csg& C = d.csgs[idx];
            const GB L = bounds(C.left, depth + 1), R = bounds(C.right, depth + 1);
            auto vol = [](const GB& q) { return (q.hi[0] - q.lo[0]) * (q.hi[1] - q.lo[1]) * (q.hi[2] - q.lo[2]); };
            if (C.op == FRAYHIP_CSG_MINUS) return L;
            if (C.op == FRAYHIP_CSG_AND) { if (L.ok && R.ok) return vol(L) <= vol(R) ? L : R; return L.ok ? L : R; }
            if (!L.ok || !R.ok) { b.ok = false; return b; }
            for (int k = 0; k < 3; k++) { b.lo[k] = std::min(L.lo[k], R.lo[k]); b.hi[k] = std::max(L.hi[k], R.hi[k]); }
        } else b.ok = false;
        for (int k = 0; k < 3; k++) if (!(std::isfinite(b.lo[k]) && std::isfinite(b.hi[k]) && b.lo[k] <= b.hi[k])) b.ok = false;
        return b;
    };
    std::vector<GB> csgLocal(d.n_nodes, GB{false, {0, 0, 0}, {0, 0, 0}});
    for (int i = 0; i < d.n_nodes; i++) {
        DNodeX& X = nodesX[i];
        for (int k = 0; k < 3; k++) X.cc[k] = X.ch[k] = 0;
        X.cM = 0; X.csgBox = 0; X.padX = 0;
        if (nodes[i].geomKind != FRAYHIP_GEOM_CSG) continue;
        const GB b = bounds(d.nodes[i].geom, 0);
        if (!b.ok) continue;
        csgLocal[i] = b;
        for (int k = 0; k < 3; k++) {
            X.cc[k] = 0.5 * (b.lo[k] + b.hi[k]);
            X.ch[k] = std::max(b.hi[k] - X.cc[k], X.cc[k] - b.lo[k]) * (1.0 + 1e-12) + 1e-5;       // the true extents and dev_misscert.hpp's constant margin
            X.cM = std::max(X.cM, std::fabs(X.cc[k]) + X.ch[k]);
        }
        X.csgBox = X.cM < 1e9 ? 1 : 0;
    }
    // Nodes a next-event segment may skip by the planes of their triangles (dev_segcert.hpp): untransformed meshes without a KD-tree and too small for a gate,
    // every triangle with finite, bounded coordinates and a normal that is not (nearly) zero.  Triangles whose N and fl(N . A) are equal bit for bit share a
    // plane entry (a planar quad is one plane).  A scene that would need more entries or nodes than the tables hold gets none.
    int nSegPlanes = 0, nSegNodes = 0;
    {
        DSegPlane planes[FRAY_SEG_MAX_PLANES];
        double planeAmax[FRAY_SEG_MAX_PLANES];
        uint32_t masks[FRAY_SEG_MAX_NODES];
        int segNodeOf[FRAY_SEG_MAX_NODES];
        bool fits = true;
        for (int i = 0; i < d.n_nodes && fits; i++) {
            const DNode& N = nodes[i];
            if (!(N.tlTris > 0 && N.tlTris < FRAY_GATE_MIN_TRIS && N.xfIdentity)) continue;
            const DTri* const tris = (const DTri*)tab[meshTables[N.geomIndex].tris];      // N = the triangle's ABcrossAC, A = its first vertex (arena_build)
            bool ok = true;
            for (int t = 0; t < N.tlTris && ok; t++) ok = segcert_triangle_ok(tris[t].N, tris[t].A);
            if (!ok) continue;
            if (nSegNodes == FRAY_SEG_MAX_NODES) { fits = false; break; }
            uint32_t mask = 0;
            for (int t = 0; t < N.tlTris; t++) {
                const double* TN = tris[t].N;
                const double* TA = tris[t].A;
                const double k = segcert_offset(TN, TA), am = std::max(std::fabs(TA[0]), std::max(std::fabs(TA[1]), std::fabs(TA[2])));
                int p = 0;
                while (p < nSegPlanes && (memcmp(planes[p].N, TN, 3 * sizeof(double)) != 0 || memcmp(&planes[p].k, &k, sizeof k) != 0)) p++;
                if (p == nSegPlanes) {
                    if (nSegPlanes == FRAY_SEG_MAX_PLANES) { fits = false; break; }
                    memcpy(planes[p].N, TN, 3 * sizeof(double)); planes[p].k = k; planeAmax[p] = 0;
                    nSegPlanes++;
                }
                planeAmax[p] = std::max(planeAmax[p], am);
                mask |= 1u << p;
            }
            if (!fits) break;
            segNodeOf[nSegNodes] = i;
            masks[nSegNodes++] = mask;
        }
        if (!fits) nSegPlanes = nSegNodes = 0;
        for (int p = 0; p < nSegPlanes; p++) { const DSegPlane q = planes[p]; segcert_make(planes[p], q.N, q.k, planeAmax[p]); }
        for (int j = 0; j < nSegNodes; j++) nodes[segNodeOf[j]].segNode = j + 1;
        memset(tab[F.tSegPlanes], 0, FRAY_SEG_MAX_PLANES * sizeof(DSegPlane));
        memset(tab[F.tSegMasks], 0, FRAY_SEG_MAX_NODES * sizeof(uint32_t));
        if (nSegPlanes) memcpy(tab[F.tSegPlanes], planes, (size_t)nSegPlanes * sizeof(DSegPlane));
        if (nSegNodes) memcpy(tab[F.tSegMasks], masks, (size_t)nSegNodes * sizeof(uint32_t));
    }
    if (!nodesX.empty()) memcpy(tab[F.tNodesX], nodesX.data(), nodesX.size() * sizeof(DNodeX));
    // gates: world-space boxes of the meshes whose brute-force triangle loops are worth skipping for a whole wave (dev_scene.hpp DGate):
    // the eight corners of the mesh's box through the node's transform (Transform::transformPoint, matrix.cpp:137-146), a hair wider
    int nGates = 0, nTight = 0;
    bool gatesExact = false;
    {
        DGate gates[FRAY_MAX_GATES], tight[FRAY_MAX_GATES];
        int gateNode[FRAY_MAX_GATES];
        // ... and of the CsgOp nodes whose tree is bounded (their machine is the most expensive thing a ray can enter), unless the box is so large
        // against the others that nearly every ray enters it anyway (a floor slab): larger than 30 times the smallest such box in some extent
        double smallest = 1e300;
        for (int i = 0; i < d.n_nodes; i++)
            if (csgLocal[i].ok) for (int k = 0; k < 3; k++) smallest = std::min(smallest, std::max(csgLocal[i].hi[k] - csgLocal[i].lo[k], 1e-9));
        for (int i = 0; i < d.n_nodes && nGates < FRAY_MAX_GATES; i++) {
            const DNode& N = nodes[i];
            double bmin[3], bmax[3];
            if (N.tlTris >= FRAY_GATE_MIN_TRIS) { put3(bmin, N.bmin); put3(bmax, N.bmax); }
            else if (csgLocal[i].ok) {
                bool huge = false;
                for (int k = 0; k < 3; k++) { bmin[k] = csgLocal[i].lo[k]; bmax[k] = csgLocal[i].hi[k]; huge = huge || bmax[k] - bmin[k] > 30.0 * smallest; }
                if (huge) continue;
            } else continue;
            DGate g;
            for (int k = 0; k < 3; k++) { g.lo[k] = 1e300; g.hi[k] = -1e300; }
            for (int c = 0; c < 8; c++) {
                const double p[3] = {c & 1 ? bmax[0] : bmin[0], c & 2 ? bmax[1] : bmin[1], c & 4 ? bmax[2] : bmin[2]};
                for (int k = 0; k < 3; k++) {
                    const double w = p[0] * N.T.m[k] + p[1] * N.T.m[3 + k] + p[2] * N.T.m[6 + k] + N.T.off[k];
                    g.lo[k] = std::min(g.lo[k], w); g.hi[k] = std::max(g.hi[k], w);
                }
            }
            // an untransformed node: the box is the geometry's own, in the space the reference tests it in -- the producers' FP32 certificate applies
            g.exact = N.xfIdentity ? 1 : 0;
            g.Mf = 0;
            for (int k = 0; k < 3; k++) {
                const double c = 0.5 * (bmin[k] + bmax[k]), half = std::max(bmax[k] - c, c - bmin[k]);
                g.cf[k] = (float)c;
                g.hf[k] = std::nextafterf((float)(half * (1.0 + 1e-12) + 1e-5 + std::fabs(c - (double)g.cf[k])), INFINITY);
                g.Mf = std::max(g.Mf, std::nextafterf(std::fabs(g.cf[k]) + g.hf[k], INFINITY));
            }
            if (!(g.Mf < 1e9f)) g.exact = 0;
            g.guard = 0; g.nDirs = 0;
            for (int j = 0; j < FRAY_GATE_MAX_DIRS; j++) g.nf[j][0] = g.nf[j][1] = g.nf[j][2] = 0;
            for (int k = 0; k < 3; k++) { const double e = 1e-6 * (1.0 + std::fabs(g.lo[k]) + std::fabs(g.hi[k])); g.lo[k] -= e; g.hi[k] += e; }
            // ... and its entry in the table's tight half: for an exact gate that stands for a mesh whose every triangle is admissible (dev_gatecert.hpp) the box of
            // the triangles themselves -- the reference's box above also holds the OBJ loader's dummy vertex (0, 0, 0) -- and the guard; else the same entry again
            tight[nGates] = g;
            if (g.exact && N.tlTris >= FRAY_GATE_MIN_TRIS && N.tlTris <= FRAY_GATECERT_MAX_TRIS) {
                const DTri* const tris = (const DTri*)tab[meshTables[N.geomIndex].tris];
                GateTri gt[FRAY_GATECERT_MAX_TRIS];
                for (int t = 0; t < N.tlTris; t++) gt[t] = GateTri{tris[t].A, tris[t].AB, tris[t].AC, tris[t].N};
                DGateTight T;
                if (gatecert_make(T, gt, N.tlTris)) {
                    DGate& o = tight[nGates];
                    for (int k = 0; k < 3; k++) { o.cf[k] = T.cf[k]; o.hf[k] = T.hf[k]; }
                    o.Mf = T.Mf; o.guard = T.guard; o.nDirs = T.nDirs;
                    memcpy(o.nf, T.nf, sizeof o.nf);
                    nTight++;
                }
            }
            gateNode[nGates] = i;
            gates[nGates++] = g;
        }
        gatesExact = nGates > 0;
        for (int q = 0; q < nGates; q++) gatesExact = gatesExact && gates[q].exact;
        if (gatesExact)
            for (int q = 0; q < nGates; q++) nodes[gateNode[q]].gated = 1;
        memset(tab[F.tGates], 0, 2 * FRAY_MAX_GATES * sizeof(DGate));
        if (nGates) memcpy(tab[F.tGates], gates, (size_t)nGates * sizeof(DGate));
        if (nGates) memcpy(tab[F.tGates] + FRAY_MAX_GATES * sizeof(DGate), tight, (size_t)nGates * sizeof(DGate));
    }
    // Miss records of the first bounce (dev_scene.hpp DCamSkip): every untransformed tree-less mesh node of at most FRAY_GATECERT_MAX_TRIS triangles whose index a
    // 32-bit word holds and which gatecert_make accepts -- no FRAY_GATE_MIN_TRIS floor, a two-triangle wall qualifies -- in node order, FRAY_CAMSKIP_MAX at most.
    // Made from the DTri table like the tight entries above; the gate table, `gated` and the segment planes do not know of them.
    int nCamSkip = 0;
    {
        DCamSkip recs[FRAY_CAMSKIP_MAX];
        memset(recs, 0, sizeof recs);
        for (int i = 0; i < d.n_nodes && i < 32 && nCamSkip < FRAY_CAMSKIP_MAX; i++) {
            const DNode& N = nodes[i];
            if (!(N.tlTris > 0 && N.tlTris <= FRAY_GATECERT_MAX_TRIS && N.xfIdentity)) continue;
            const DTri* const tris = (const DTri*)tab[meshTables[N.geomIndex].tris];
            GateTri gt[FRAY_GATECERT_MAX_TRIS];
            for (int t = 0; t < N.tlTris; t++) gt[t] = GateTri{tris[t].A, tris[t].AB, tris[t].AC, tris[t].N};
            DGateTight T;
            if (!gatecert_make(T, gt, N.tlTris)) continue;
            DCamSkip& o = recs[nCamSkip++];
            for (int k = 0; k < 3; k++) { o.cf[k] = T.cf[k]; o.hf[k] = T.hf[k]; }
            o.Mf = T.Mf; o.guard = T.guard; o.nDirs = T.nDirs; o.node = i;
            memcpy(o.nf, T.nf, sizeof o.nf);
        }
        memcpy(tab[F.tCamSkip], recs, sizeof recs);
    }
    F.nCamSkip = nCamSkip;
    // Shade shortcuts (frayhip_scene_shade_shortcuts; dev_scene.hpp DScene::shadeIdentity, lightsDiagonal).  The world-normal table: for every node that is an
    // untransformed flat mesh kept with its triangles (arena_keeps_tris), whose shader reads no (u, v) and which has no bump texture, entry i * normStride + t is
    // what finalize_hit makes of triangle t's normal; every other entry is zero.  shadeIdentity: every node is such a node.
    {
        const size_t entries = (size_t)d.n_nodes * (size_t)F.normStride;
        double* const wn = (double*)tab[F.tWorldNormals];
        if (entries) memset(wn, 0, entries * 3 * sizeof(double));
        bool all = entries > 0;
        for (int i = 0; i < d.n_nodes && entries; i++) {
            const DNode& N = nodes[i];
            bool ok = N.xfIdentity && N.geomKind == FRAYHIP_GEOM_MESH && N.bumpTex < 0 && !shaders[N.shader].usesUV;
            if (ok) { const DMesh& M = meshes[N.geomIndex]; ok = arena_keeps_tris(M) && !M.smooth && M.nTris <= F.normStride; }
            all = all && ok;
            if (!ok) continue;
            const DTri* const tris = (const DTri*)tab[meshTables[N.geomIndex].tris];
            for (int t = 0; t < meshes[N.geomIndex].nTris; t++) world_normal(tris[t].g, N.T.m, wn + 3 * ((size_t)i * F.normStride + t));
        }
        F.shadeIdentity = all ? 1 : 0;
    }
    // lightsDiagonal: every light is one light_is_diagonal accepts
    {
        bool all = d.n_lights > 0;
        for (int i = 0; i < d.n_lights; i++) all = all && light_is_diagonal(d.lights[i]);
        F.lightsDiagonal = all ? 1 : 0;
    }
    if (!nodes.empty()) memcpy(tab[F.tNodes], nodes.data(), nodes.size() * sizeof(DNode));
    if (!tex.empty()) memcpy(tab[F.tTex], tex.data(), tex.size() * sizeof(DTexture));

    F.nGates = nGates; F.gatesExact = gatesExact ? 1 : 0; F.nTightGates = nTight;
    F.nSegPlanes = nSegPlanes; F.nSegNodes = nSegNodes;
    // Certified segments (kernels.hpp path_shade, dev_trace.hpp segment_certified): EVERY node is one a next-event segment can be proven to pass -- by the planes
    // of its triangles (segNode) or by its exact gate (gated, which implies gatesExact).  Any other node (a sphere, a plane, a Cube / CSG node without a gate, a
    // transformed or a KD mesh, a scene with too many planes, nodes or gates for the tables, an inexact gate) clears it.  Recomputed here with the tables it
    // follows from, so an updated arena (arena_update) carries the flag of its own nodes.
    bool segCertAll = true;
    for (int i = 0; i < d.n_nodes; i++) segCertAll = segCertAll && (nodes[i].segNode != 0 || nodes[i].gated != 0);
    // ... and every plane entry can pass for SOME next-event segment.  Such a segment ends on a light, and the rule needs every entry: an entry in whose plane
    // every light lies whole (a point light's position, a RectLight's four corners -- its samples are convex combinations of them -- all within t0 of it,
    // the least margin seg_same_side asks of an end) passes for no segment, and path_shade would evaluate the certificate for nothing.  Without a light there
    // are no segments.  The lights are this function's too, so a moved light (arena_update) changes the flag like a moved node.
    segCertAll = segCertAll && d.n_lights > 0;
    const DSegPlane* const entries = (const DSegPlane*)tab[F.tSegPlanes];
    for (int p = 0; p < nSegPlanes && segCertAll; p++) {
        const DSegPlane& P = entries[p];
        bool off = false;               // some light has a point off this plane
        for (int i = 0; i < d.n_lights && !off; i++) {
            const frayhip_light& l = d.lights[i];
            for (int c = 0; c < (l.kind == FRAYHIP_LIGHT_RECT ? 4 : 1) && !off; c++) {
                const double px = c & 1 ? 0.5 : -0.5, pz = c & 2 ? 0.5 : -0.5;          // light_nth_sample (dev_shade.hpp): (px, 0, pz) through T
                double w[3];
                for (int k = 0; k < 3; k++) w[k] = l.kind == FRAYHIP_LIGHT_RECT ? px * l.T.m[k] + pz * l.T.m[6 + k] + l.T.offset[k] : l.pos[k];
                off = std::fabs(P.N[0] * w[0] + P.N[1] * w[1] + P.N[2] * w[2] - P.k) > P.t0;
            }
        }
        segCertAll = off;
    }
    // ... and a segment STARTS 1e-6 off the surface it was sampled on (dev_shade.hpp nee_prepare: a = x + norm * 1e-6).  On a gated node that start lies inside
    // the gate; on a plane node it clears the node's own planes only where 1e-6 |N|_2 exceeds their margin (at least t0, which grows with the coordinates: in a
    // room of extent 5e6 it is 1e-4 |N|_2).  Some plane node must be able to start a certified segment, or none exists.
    const uint32_t* const nodeMasks = (const uint32_t*)tab[F.tSegMasks];
    bool starts = false;
    for (int j = 0; j < nSegNodes && !starts; j++) {
        bool clear = true;
        for (int p = 0; p < nSegPlanes; p++)
            if (nodeMasks[j] >> p & 1u) {
                const DSegPlane& P = entries[p];
                clear = clear && 1e-6 * std::sqrt(P.N[0] * P.N[0] + P.N[1] * P.N[1] + P.N[2] * P.N[2]) > P.t0;
            }
        starts = clear;
    }
    segCertAll = segCertAll && starts;
    F.segCertAll = segCertAll ? 1 : 0;
}

}  // namespace detail

// `d` has passed frayhip_scene_create's validation (every index in range, CSG trees at most FRAY_CSG_DEPTH deep).
inline void arena_build(const frayhip_scene_desc& d, ArenaBuilt& B)
{
    using detail::put3;
    B.host.clear(); B.tables.clear(); B.meshTables.clear(); B.texelOffset.clear();
    ArenaFacts& F = B.F;
    memset(&F, 0, sizeof F);
    detail::Arena A{B.host, B.tables};
    // the tables that the editable part of a description decides are laid out here, zero-filled, and written by detail::fill_editable below -- the
    // function arena_update runs again
    A.reserve((size_t)d.n_nodes * sizeof(DNode));                             // (tree-less nodes hold a pointer: arena_place)
    F.tNodes = A.last();
    A.reserve((size_t)d.n_nodes * sizeof(DNodeX));
    F.tNodesX = A.last();
    A.reserve(2 * FRAY_MAX_GATES * sizeof(DGate));                            // the path tracer's gates (DGate), as they are and in their tight form
    F.tGates = A.last();
    A.reserve(FRAY_SEG_MAX_PLANES * sizeof(DSegPlane));                       // the planes shadow segments are certified against (dev_segcert.hpp)
    F.tSegPlanes = A.last();
    A.reserve(FRAY_SEG_MAX_NODES * sizeof(uint32_t));
    F.tSegMasks = A.last();
    A.reserve((size_t)d.n_planes * sizeof(DPlane));
    F.tPlanes = A.last();
    A.reserve((size_t)d.n_spheres * sizeof(DSphere));
    F.tSpheres = A.last();
    A.reserve((size_t)d.n_cubes * sizeof(DCube));
    F.tCubes = A.last();
    std::vector<DCsg> csgs(d.n_csgs);
    for (int i = 0; i < d.n_csgs; i++) {
        const frayhip_csg& g = d.csgs[i];
        csgs[i].op = g.op;
        csgs[i].leftKind = d.geoms[g.left].kind; csgs[i].leftIndex = d.geoms[g.left].index; csgs[i].leftGeom = g.left;
        csgs[i].rightKind = d.geoms[g.right].kind; csgs[i].rightIndex = d.geoms[g.right].index; csgs[i].rightGeom = g.right;
        csgs[i].flat = (csgs[i].leftKind <= FRAYHIP_GEOM_CUBE && csgs[i].rightKind <= FRAYHIP_GEOM_CUBE) ? 1 : 0;
    }
    A.add(csgs.data(), csgs.size() * sizeof(DCsg));
    F.tCsgs = A.last();
    // meshes
    std::vector<DMesh> meshes(d.n_meshes);
    B.meshTables.resize(d.n_meshes);
    for (int mi = 0; mi < d.n_meshes; mi++) {
        const frayhip_mesh& m = d.meshes[mi];
        DMesh& M = meshes[mi];
        put3(M.bmin, m.bbox_min);
        put3(M.bmax, m.bbox_max);
        M.boxMax = 0;
        for (int k = 0; k < 3; k++) M.boxMax = std::max(M.boxMax, std::max(std::fabs(m.bbox_min[k]), std::fabs(m.bbox_max[k])));
        M.nTris = m.n_triangles;
        M.hasKd = m.has_kd;
        if (m.has_kd) F.kdMeshes = 1;
        M.smooth = !(m.faceted || m.n_normals == 0);
        M.culling = m.backfaceCulling;
        M.hasUV = m.n_uvs != 0;
        std::vector<DTri> tris(m.n_triangles);
        std::vector<DTriAttr> attrs(m.n_triangles);
        for (int t = 0; t < m.n_triangles; t++) {
            const frayhip_triangle& T = m.triangles[t];
            DTri& o = tris[t];
            put3(o.g, T.gnormal);
            put3(o.A, m.vertices + 3 * (size_t)T.v[0]);
            put3(o.N, T.ABcrossAC);
            put3(o.AC, T.AC);
            put3(o.AB, T.AB);
            o.index = t; o.pad = 0;
            DTriAttr& a = attrs[t];
            memset(&a, 0, sizeof a);
            if (M.smooth) {
                put3(a.nA, m.normals + 3 * (size_t)T.n[0]);
                put3(a.nB, m.normals + 3 * (size_t)T.n[1]);
                put3(a.nC, m.normals + 3 * (size_t)T.n[2]);
            }
            if (M.hasUV) {
                const double* tA = m.uvs + 3 * (size_t)T.t[0]; const double* tB = m.uvs + 3 * (size_t)T.t[1]; const double* tC = m.uvs + 3 * (size_t)T.t[2];
                a.tA[0] = tA[0]; a.tA[1] = tA[1]; a.tB[0] = tB[0]; a.tB[1] = tB[1]; a.tC[0] = tC[0]; a.tC[1] = tC[1];
            }
            put3(a.dNdx, T.dNdx);
            put3(a.dNdy, T.dNdy);
        }
        // KD nodes: add each node's own box.  Boxes are derived top-down exactly as BBox::split
        // does (copy parent, overwrite one coordinate).
        std::vector<DKd> kd(m.n_kdnodes);
        std::vector<DKdBox> kdBox(m.n_kdnodes);
        if (m.n_kdnodes > 0) {
            for (int k = 0; k < 3; k++) { kdBox[0].lo[k] = m.bbox_min[k]; kdBox[0].hi[k] = m.bbox_max[k]; }
            for (int n = 0; n < m.n_kdnodes; n++) {   // parents precede children in the array
                const frayhip_kdnode& K = m.kdnodes[n];
                DKd& o = kd[n];
                o.child0 = K.child0; o.meta = K.axis;
                if (K.axis != 3) {
                    o.split = K.split;
                    o.meta |= (m.kdnodes[K.child0].axis == 3 ? 4 : 0) | (m.kdnodes[K.child0 + 1].axis == 3 ? 8 : 0);
                    kdBox[K.child0] = kdBox[n];
                    kdBox[K.child0 + 1] = kdBox[n];
                    kdBox[K.child0].hi[K.axis] = K.split;
                    kdBox[K.child0 + 1].lo[K.axis] = K.split;
                } else {
                    o.triBegin = K.tri_begin; o.triCount = K.tri_count;
                }
            }
        }
        ArenaMeshTables& MT = B.meshTables[mi];
        A.add(tris.data(), tris.size() * sizeof(DTri)); MT.tris = A.last();
        A.add(attrs.data(), attrs.size() * sizeof(DTriAttr)); MT.attrs = A.last();
        A.add(kd.data(), kd.size() * sizeof(DKd)); MT.kd = A.last();
        A.add(kdBox.data(), kdBox.size() * sizeof(DKdBox)); MT.kdBox = A.last();
        A.add(m.trirefs, (size_t)m.n_trirefs * sizeof(int32_t)); MT.refs = A.last();
        std::vector<DTri> ltris((size_t)m.n_trirefs);
        for (int r = 0; r < m.n_trirefs; r++) ltris[r] = tris[m.trirefs[r]];
        A.add(ltris.data(), ltris.size() * sizeof(DTri)); MT.ltris = A.last();
        // the same leaf order again as FP32 records of the certified filter (dev_tricert.hpp), relative to the centre of the mesh's box
        for (int k = 0; k < 3; k++) M.ref[k] = (m.bbox_min[k] + m.bbox_max[k]) * 0.5;
        std::vector<DTri32> l32(ltris.size());
        for (size_t r = 0; r < ltris.size(); r++) tricert_make(l32[r], ltris[r].A, ltris[r].AB, ltris[r].AC, ltris[r].N, M.ref);
        A.add(l32.data(), l32.size() * sizeof(DTri32)); MT.ltris32 = A.last();
    }
    A.add(d.texels, (size_t)d.n_texels * sizeof(float));
    F.tTexels = A.last();
    B.texelOffset.resize(d.n_textures);
    for (int i = 0; i < d.n_textures; i++) B.texelOffset[i] = d.textures[i].texel_offset;
    A.reserve((size_t)d.n_shaders * sizeof(DShader));
    F.tShaders = A.last();
    A.reserve((size_t)d.n_layers * sizeof(DLayer));
    F.tLayers = A.last();
    A.reserve((size_t)d.n_lights * sizeof(DLight));
    F.tLights = A.last();
    size_t oMeshes = A.reserve(meshes.size() * sizeof(DMesh));              // the tables that hold pointers: written here with the pointers null
    F.tMeshes = A.last();
    A.reserve((size_t)d.n_textures * sizeof(DTexture));
    F.tTex = A.last();
    if (!meshes.empty()) memcpy(A.host.data() + oMeshes, meshes.data(), meshes.size() * sizeof(DMesh));
    A.reserve(FRAY_CAMSKIP_MAX * sizeof(DCamSkip));                           // the first bounce's miss records (DCamSkip): last, so that every other table stands where it stood
    F.tCamSkip = A.last();
    // the world-normal table of the shade shortcuts (fill_editable): one entry per node and triangle, FRAY_GATECERT_MAX_TRIS triangles per node -- what a mesh kept
    // with its triangles has at most; a node's geometry is editable, and like every editable table this one does not grow with a mesh.  After every other table,
    // which stand where they stood.  None for a scene of more than 4096 nodes (3 MiB; finalize_hit indexes it with 32-bit arithmetic).
    F.normStride = d.n_nodes <= 4096 ? FRAY_GATECERT_MAX_TRIS : 0;
    A.reserve((size_t)d.n_nodes * (size_t)F.normStride * 3 * sizeof(double));
    F.tWorldNormals = A.last();

    F.nNodes = d.n_nodes; F.nLights = d.n_lights; F.nMeshes = d.n_meshes; F.nTextures = d.n_textures;
    F.envPresent = d.environment.present;
    F.envLoaded = d.environment.loaded;
    if (d.n_textures > 0 || (d.environment.present && d.environment.loaded)) F.textured = 1;
    for (int f = 0; f < 6; f++) {
        F.envWidth[f] = d.environment.width[f];
        F.envHeight[f] = d.environment.height[f];
        F.envTexelOffset[f] = d.environment.texel_offset[f];
    }
    std::vector<unsigned char*> tab(B.tables.size());
    for (size_t t = 0; t < B.tables.size(); t++) tab[t] = B.host.data() + B.tables[t].off;
    detail::fill_editable(d, B.meshTables.data(), F, tab.data());
}

// The editable part of `d` written again into an arena built earlier (frayhip_scene_update; `d` has passed its checks: the fixed part is what it was at
// arena_build, the editable part in range).  tab[t]: where table t can be written -- needed for the tables of arena_editable_tables, and to be read for the
// DMesh table and the DTri table of every mesh with detail::arena_keeps_tris; the others may be null.  F: the facts of the arena as built, updated in place.
inline void arena_update(const frayhip_scene_desc& d, const ArenaMeshTables* meshTables, ArenaFacts& F, unsigned char* const* tab)
{
    detail::fill_editable(d, meshTables, F, tab);
}
// ... on the arena itself, inner pointers null as arena_build left them
inline void arena_update(const frayhip_scene_desc& d, ArenaBuilt& B)
{
    std::vector<unsigned char*> tab(B.tables.size());
    for (size_t t = 0; t < B.tables.size(); t++) tab[t] = B.host.data() + B.tables[t].off;
    arena_update(d, B.meshTables.data(), B.F, tab.data());
}
// the tables arena_update writes: none of them grows with a mesh or with the texel pool
inline std::vector<int32_t> arena_editable_tables(const ArenaFacts& F)
{
    return {F.tNodes, F.tNodesX, F.tGates, F.tSegPlanes, F.tSegMasks, F.tPlanes, F.tSpheres, F.tCubes, F.tShaders, F.tLayers, F.tLights, F.tTex, F.tCamSkip, F.tWorldNormals};
}

// write[t]: where table t can be written now (the staging copy, or the table itself); addr[t]: where the kernels, or the host harness, will find it.
// Every pointer stored is addr[..] (+ an offset inside the texel pool); nothing is read through addr.  Fills every field of S that a description
// decides; the per-frame ones (ambient, maxTraceDepth, gi, saturation, the two options) are frame_scene's.
inline void arena_place(const ArenaFacts& F, const ArenaMeshTables* meshTables, const int64_t* texelOffset, unsigned char* const* write,
                        const unsigned char* const* addr, DScene& S)
{
    DMesh* const meshes = (DMesh*)write[F.tMeshes];
    for (int mi = 0; mi < F.nMeshes; mi++) {
        const ArenaMeshTables& MT = meshTables[mi];
        meshes[mi].tris = (const FRAY_RO DTri*)addr[MT.tris];
        meshes[mi].attrs = (const FRAY_RO DTriAttr*)addr[MT.attrs];
        meshes[mi].kd = (const FRAY_RO DKd*)addr[MT.kd];
        meshes[mi].kdBox = (const FRAY_RO DKdBox*)addr[MT.kdBox];
        meshes[mi].refs = (const FRAY_RO int32_t*)addr[MT.refs];
        meshes[mi].ltris = (const FRAY_RO DTri*)addr[MT.ltris];
        meshes[mi].ltris32 = (const FRAY_RO DTri32*)addr[MT.ltris32];
    }
    DNode* const nodes = (DNode*)write[F.tNodes];
    for (int i = 0; i < F.nNodes; i++)
        if (nodes[i].geomKind == FRAYHIP_GEOM_MESH && !meshes[nodes[i].geomIndex].hasKd) nodes[i].tlPtr = meshes[nodes[i].geomIndex].tris;
    DTexture* const tex = (DTexture*)write[F.tTex];
    for (int i = 0; i < F.nTextures; i++) tex[i].texels = (const FRAY_RO float*)addr[F.tTexels] + texelOffset[i];

    S.nodes = (const FRAY_RO DNode*)addr[F.tNodes];
    S.nodesX = (const FRAY_RO DNodeX*)addr[F.tNodesX];
    S.gates = (const FRAY_RO DGate*)addr[F.tGates];
    S.nGates = F.nGates; S.gatesExact = F.gatesExact;
    S.segPlanes = (const FRAY_RO DSegPlane*)addr[F.tSegPlanes];
    S.segNodeMasks = (const FRAY_RO uint32_t*)addr[F.tSegMasks];
    S.nSegPlanes = F.nSegPlanes; S.nSegNodes = F.nSegNodes; S.segCertAll = F.segCertAll;
    S.camSkip = (const FRAY_RO DCamSkip*)addr[F.tCamSkip];
    S.nCamSkip = F.nCamSkip; S.padCamSkip = 0;
    S.worldNormals = (const FRAY_RO double*)addr[F.tWorldNormals];
    S.normStride = F.normStride; S.shadeIdentity = F.shadeIdentity; S.lightsDiagonal = F.lightsDiagonal; S.subdShift = 1;
    S.planes = (const FRAY_RO DPlane*)addr[F.tPlanes];
    S.spheres = (const FRAY_RO DSphere*)addr[F.tSpheres];
    S.cubes = (const FRAY_RO DCube*)addr[F.tCubes];
    S.csgs = (const FRAY_RO DCsg*)addr[F.tCsgs];
    S.meshes = (const FRAY_RO DMesh*)addr[F.tMeshes];
    S.shaders = (const FRAY_RO DShader*)addr[F.tShaders];
    S.layers = (const FRAY_RO DLayer*)addr[F.tLayers];
    S.textures = (const FRAY_RO DTexture*)addr[F.tTex];
    S.lights = (const FRAY_RO DLight*)addr[F.tLights];
    S.env.present = F.envPresent;
    S.env.loaded = F.envLoaded;
    for (int f = 0; f < 6; f++) {
        S.env.width[f] = F.envWidth[f];
        S.env.height[f] = F.envHeight[f];
        S.env.face[f] = (const FRAY_RO float*)addr[F.tTexels] + F.envTexelOffset[f];
    }
    S.nNodes = F.nNodes;
    S.nLights = F.nLights;
    S.probPickLight = F.nLights > 0 ? 1.0f / (float)F.nLights : 0.0f;
}

}  // namespace frayhip_arena
