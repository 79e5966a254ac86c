// Test harness (CPU only), second half of the host lane (tests/test_trace_host.py): the device's traversal code -- closest_hit, node_intersect, the
// KD walk, the CSG paths, finalize_hit, light_record, visible and the segment-plane copy of visible with segment_skip_nodes (fray_amd/csrc/dev_trace.hpp,
// dev_shade.hpp) -- compiled for the host as one lane of a wave, over a stand-in <hip/hip_runtime.h>, so that MemorySanitizer, AddressSanitizer and
// UndefinedBehaviorSanitizer see it run.  Not one device header is edited for it.
// usage: trace_host ARENA RAYS RESULT      (formats: hostlane_format.h)
// C-style I/O only: under MemorySanitizer every byte of the scene comes from fread, and no uninstrumented library code touches the harness's data.
// Every table of the arena goes into a heap block of its own (arena_place): an index past a table's end is an error, not a read of its neighbour.
#include <hip/hip_runtime.h>      // the stand-in of this directory

#include <float.h>
#include <stdio.h>
#include <stdlib.h>

#include "dev_shade.hpp"          // dev_math, dev_scene, dev_trace, dev_sort, the certificates, dev_rng, dev_trig
#include "scene_arena.hpp"
#include "hostlane_format.h"

// dev_math.hpp only declares these two on a host pass: a wave of one lane
lanes_t lanes(bool p) { return p ? 1ull : 0ull; }
bool lane_of(lanes_t m) { return (m & 1ull) != 0; }

#if defined(__has_feature)
#if __has_feature(memory_sanitizer)
#include <sanitizer/msan_interface.h>
#define HOSTLANE_MSAN 1
#endif
#endif
// HOSTLANE_SELFTEST (tests/test_trace_host.py builds these to show that the sanitizers see what they are there for; never otherwise):
//   1: the node loop runs one node past the end of the node table;  2: a ray whose origin has x == 12345 is not traced and a field of its record that
//   nothing wrote reaches the output
#ifndef HOSTLANE_SELFTEST
#define HOSTLANE_SELFTEST 0
#endif
#ifndef HOSTLANE_POISON_BYTE
#define HOSTLANE_POISON_BYTE 0xA5      // the builds that are compared with each other take different bytes: a result made of poison differs between them
#endif
// What a local holds before the code under test has written it: MemorySanitizer's "uninitialised", elsewhere a byte pattern.
template <class T> static void poison(T& v)
{
#ifdef HOSTLANE_MSAN
    __msan_poison(&v, sizeof v);
#else
    memset((void*)&v, HOSTLANE_POISON_BYTE, sizeof v);
#endif
}

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool put(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
static void* block(size_t bytes)
{
    void* p = nullptr;
    if (posix_memalign(&p, 256, bytes) != 0) { fprintf(stderr, "trace_host: out of memory\n"); exit(2); }
    return p;
}
static int fail(const char* what) { fprintf(stderr, "trace_host: %s\n", what); return 2; }

static Cnt zero_counters()
{
    Cnt c;
    c.closest = c.shadow = c.node = c.kdInner = c.leafRefs = c.tri = c.prim = c.smooth = c.samples = c.tex = 0;
    c.envelope = 0;
    return c;
}
static void counters_out(const Cnt& c, uint64_t* o)
{
    o[0] = c.closest; o[1] = c.shadow; o[2] = c.node; o[3] = c.kdInner; o[4] = c.leafRefs; o[5] = c.tri; o[6] = c.prim; o[7] = c.smooth; o[8] = c.samples;
    o[9] = c.tex; o[10] = c.envelope;
}

// the ray queries' own filter (query_variant.hip): what fails it is a miss / visible and is not traced
static bool finite3(V3 v) { return fabs(v.x) <= DBL_MAX && fabs(v.y) <= DBL_MAX && fabs(v.z) <= DBL_MAX; }

// One ray as k_query_closest<ST, true> answers it: the id and the nine doubles of the record.
template <int ST>
static void closest_record(const DScene& S, V3 o, V3 d, Cnt& c, int32_t& id, double* rec)
{
    const double dd = d.x * d.x + d.y * d.y + d.z * d.z;
    HitT<ST> h;
    poison(h);
    h.node = -1;
    h.dist = 1e99;
#if HOSTLANE_SELFTEST == 2
    if (finite3(o) && dd > 0.0 && dd <= DBL_MAX && o.x != 12345.0) closest_hit<ST>(S, o, d, h, c);
#else
    if (finite3(o) && dd > 0.0 && dd <= DBL_MAX) closest_hit<ST>(S, o, d, h, c);
#endif
    V3 ip = v3(0, 0, 0), norm = v3(0, 0, 0);
    double u = 0, v = 0;
    if (h.node >= 0) {
        HitInfo info;
        poison(info);
        finalize_hit<ST, false, true>(S, h, o, d, true, info);
        ip = info.ip; norm = info.norm; u = info.u; v = info.v;
    } else if (h.node <= -2) {
        poison(ip); poison(norm);
        light_record(S.lights[-2 - h.node], o, d, ip, norm);
    }
    id = h.node;          // (on a miss nothing but node and dist is read back)
    rec[0] = h.dist;
#if HOSTLANE_SELFTEST == 2
    if (h.node == -1) u = h.l2;          // the self-test build reads a field of a miss that nothing has to have written
#endif
    rec[1] = ip.x; rec[2] = ip.y; rec[3] = ip.z;
    rec[4] = norm.x; rec[5] = norm.y; rec[6] = norm.z;
    rec[7] = u; rec[8] = v;
}

template <int ST, bool SEGP>
static bool segment_visible(const DScene& S, V3 a, V3 b, Cnt& c, uint32_t* skipOut)
{
    const V3 e = b - a;
    const double ll = e.x * e.x + e.y * e.y + e.z * e.z;
    if (skipOut) *skipOut = 0;
    if (!(finite3(a) && finite3(b) && ll > 0.0 && ll <= DBL_MAX)) return true;
    if constexpr (SEGP) {
        // k_pt_shadow's order: the whole wave (here: the one live lane) evaluates the certificate, then visible() with the nodes to skip
        uint32_t skip;
        poison(skip);
        skip = segment_skip_nodes(S, a, b, true);
        *skipOut = skip;
        return visible<ST, false, true>(S, a, b, c, false, skip);
    } else {
        return visible<ST>(S, a, b, c);
    }
}

template <int W>
static int run(const DScene& S, uint64_t nRays, const double* o, const double* d, uint64_t nSegs, const double* a, const double* b, FILE* out)
{
    constexpr bool SEGP = W == 0 || W == 8;
    HostlaneResultHeader H;
    memset(&H, 0, sizeof H);
    memcpy(H.magic, HOSTLANE_RESULT_MAGIC, 8);
    H.word = W; H.nRays = nRays; H.nSegs = nSegs; H.segp = SEGP ? 1 : 0;
    int32_t* id = (int32_t*)block(nRays * sizeof(int32_t));
    int32_t* idC = (int32_t*)block(nRays * sizeof(int32_t));
    double* rec = (double*)block(nRays * 9 * sizeof(double));
    double* recC = (double*)block(nRays * 9 * sizeof(double));
    Cnt none = zero_counters(), cc = zero_counters();
    for (uint64_t i = 0; i < nRays; i++) {
        const V3 ro = v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        closest_record<W>(S, ro, rd, none, id[i], rec + 9 * i);
        closest_record<W | 1>(S, ro, rd, cc, idC[i], recC + 9 * i);
    }
    uint8_t* vis = (uint8_t*)block(nSegs);
    uint8_t* visC = (uint8_t*)block(nSegs);
    uint8_t* visP = (uint8_t*)block(nSegs);
    uint32_t* skip = (uint32_t*)block(nSegs * sizeof(uint32_t));
    Cnt cv = zero_counters();
    for (uint64_t i = 0; i < nSegs; i++) {
        const V3 sa = v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]), sb = v3(b[3 * i], b[3 * i + 1], b[3 * i + 2]);
        vis[i] = segment_visible<W, false>(S, sa, sb, none, nullptr) ? 1 : 0;
        visC[i] = segment_visible<W | 1, false>(S, sa, sb, cv, nullptr) ? 1 : 0;
        visP[i] = 0; skip[i] = 0;
        if constexpr (SEGP) visP[i] = segment_visible<W, true>(S, sa, sb, none, skip + i) ? 1 : 0;
    }
    uint64_t cntClosest[11], cntVisible[11];
    counters_out(cc, cntClosest);
    counters_out(cv, cntVisible);
    const bool ok = put(out, &H, sizeof H) && put(out, id, nRays * sizeof(int32_t)) && put(out, rec, nRays * 9 * sizeof(double)) &&
                    put(out, idC, nRays * sizeof(int32_t)) && put(out, recC, nRays * 9 * sizeof(double)) && put(out, cntClosest, sizeof cntClosest) &&
                    put(out, vis, nSegs) && put(out, visC, nSegs) && put(out, cntVisible, sizeof cntVisible) && put(out, visP, nSegs) &&
                    put(out, skip, nSegs * sizeof(uint32_t));
    free(id); free(idC); free(rec); free(recC); free(vis); free(visC); free(visP); free(skip);
    return ok ? 0 : fail("short write");
}

int main(int argc, char** argv)
{
    if (argc != 4) return fail("usage: trace_host ARENA RAYS RESULT");
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the arena file");
    HostlaneArenaHeader AH;
    frayhip_arena::ArenaFacts F;
    if (!get(f, &AH, sizeof AH) || memcmp(AH.magic, HOSTLANE_ARENA_MAGIC, 8) != 0 || AH.factsBytes != sizeof F || !get(f, &F, sizeof F)) return fail("bad arena file");
    if (AH.nTables > (1u << 24) || AH.nMeshes != (uint64_t)F.nMeshes || AH.nTextures != (uint64_t)F.nTextures) return fail("bad arena header");
    frayhip_arena::ArenaTable* tables = (frayhip_arena::ArenaTable*)block(AH.nTables * sizeof(frayhip_arena::ArenaTable));
    frayhip_arena::ArenaMeshTables* meshTables = (frayhip_arena::ArenaMeshTables*)block(AH.nMeshes * sizeof(frayhip_arena::ArenaMeshTables));
    int64_t* texelOffset = (int64_t*)block(AH.nTextures * sizeof(int64_t));
    if (!get(f, tables, AH.nTables * sizeof(frayhip_arena::ArenaTable)) || !get(f, meshTables, AH.nMeshes * sizeof(frayhip_arena::ArenaMeshTables)) ||
        !get(f, texelOffset, AH.nTextures * sizeof(int64_t)))
        return fail("short arena file");
    // every table into a block of exactly its size: the file holds the arena as one run of bytes, alignment gaps included
    unsigned char** where = (unsigned char**)block(AH.nTables * sizeof(unsigned char*));
    uint64_t pos = 0;
    for (uint64_t t = 0; t < AH.nTables; t++) {
        if (tables[t].off < pos || tables[t].off + tables[t].bytes > AH.arenaBytes) return fail("arena tables out of order");
        if (fseek(f, (long)(tables[t].off - pos), SEEK_CUR) != 0) return fail("seek");
        where[t] = (unsigned char*)block(tables[t].bytes);
        if (!get(f, where[t], tables[t].bytes)) return fail("short arena file");
        pos = tables[t].off + tables[t].bytes;
    }
    fclose(f);
    DScene S;
    memset(&S, 0, sizeof S);
    frayhip_arena::arena_place(F, meshTables, texelOffset, where, where, S);
    S.segmentPlanes = 1;          // option "segment_planes" (frame_scene): on, so that segment_skip_nodes certifies
#if HOSTLANE_SELFTEST == 1
    S.nNodes++;                   // the self-test build walks one node past the table's end: AddressSanitizer must say so (the tables are blocks of their own)
#endif

    f = fopen(argv[2], "rb");
    if (!f) return fail("cannot open the ray file");
    HostlaneRayHeader RH;
    if (!get(f, &RH, sizeof RH) || memcmp(RH.magic, HOSTLANE_RAYS_MAGIC, 8) != 0 || RH.nRays > (1u << 28) || RH.nSegs > (1u << 28)) return fail("bad ray file");
    double* o = (double*)block(RH.nRays * 3 * sizeof(double));
    double* d = (double*)block(RH.nRays * 3 * sizeof(double));
    double* a = (double*)block(RH.nSegs * 3 * sizeof(double));
    double* b = (double*)block(RH.nSegs * 3 * sizeof(double));
    if (!get(f, o, RH.nRays * 3 * sizeof(double)) || !get(f, d, RH.nRays * 3 * sizeof(double)) || !get(f, a, RH.nSegs * 3 * sizeof(double)) ||
        !get(f, b, RH.nSegs * 3 * sizeof(double)))
        return fail("short ray file");
    fclose(f);

    FILE* out = fopen(argv[3], "wb");
    if (!out) return fail("cannot write the result file");
    const int w = F.extGeometry ? 2 : F.kdMeshes ? 4 : F.textured ? 8 : 0;          // flag_word (entry_support.hpp)
    int rc;
    if (w == 0) rc = run<0>(S, RH.nRays, o, d, RH.nSegs, a, b, out);
    else if (w == 2) rc = run<2>(S, RH.nRays, o, d, RH.nSegs, a, b, out);
    else if (w == 4) rc = run<4>(S, RH.nRays, o, d, RH.nSegs, a, b, out);
    else rc = run<8>(S, RH.nRays, o, d, RH.nSegs, a, b, out);
    if (fclose(out) != 0 && rc == 0) rc = fail("short write");
    for (uint64_t t = 0; t < AH.nTables; t++) free(where[t]);
    free(where); free(tables); free(meshTables); free(texelOffset); free(o); free(d); free(a); free(b);
    return rc;
}
