// Test harness (CPU only) of the certified segments (tests/test_certified_segments_host.py; DESIGN.md "Certified segments"): the rule by which
// path_shade (fray_amd/csrc/kernels.hpp) stores a next-event segment's term itself instead of queueing the segment -- ray_gate_class,
// segment_certified and segment_surely_visible of fray_amd/csrc/dev_trace.hpp, the kernels' own code -- compiled for the host as one lane of a wave
// over the stand-in <hip/hip_runtime.h> of tests/native/hostlane, beside visible<0>'s answer for the same segment.
// usage: certseg_host ARENA RAYS RESULT
//   ARENA, RAYS: the host lane's files (tests/native/hostlane/hostlane_format.h; arena_dump writes the first, the rays of RAYS are ignored)
//   RESULT: "FRAYCSG1", uint64 nSegs, uint64 eligible (DScene::segCertAll), uint64 nGates, uint64 nSegPlanes, then per segment one byte each:
//           planes[nSegs]     segment_certified: the ends lie on one side of every plane entry by the margin
//           gateFree[nSegs]   the segment's ray is proven to miss every gate (or the scene has none)
//           certified[nSegs]  segment_surely_visible with both options on: what path_shade decides
//           vis[nSegs]        visible<0>
// Built with AddressSanitizer + UndefinedBehaviorSanitizer and plain; and once more with the certificates' margins removed
// (-DFRAY_SEGCERT_SCALE=0 -DFRAY_MISSCERT_SCALE=0) to show that a wrong certificate is seen.
#include <hip/hip_runtime.h>      // the stand-in of tests/native/hostlane

#include <float.h>
#include <stdio.h>
#include <stdlib.h>

#include "dev_shade.hpp"
#include "scene_arena.hpp"
#include "hostlane_format.h"

lanes_t lanes(bool p) { return p ? 1ull : 0ull; }
bool lane_of(lanes_t m) { return (m & 1ull) != 0; }

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool put(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
static void* block(size_t bytes)
{
    void* p = nullptr;
    if (posix_memalign(&p, 256, bytes ? bytes : 1) != 0) { fprintf(stderr, "certseg_host: out of memory\n"); exit(2); }
    return p;
}
static int fail(const char* what) { fprintf(stderr, "certseg_host: %s\n", what); return 2; }
static bool finite3(V3 v) { return fabs(v.x) <= DBL_MAX && fabs(v.y) <= DBL_MAX && fabs(v.z) <= DBL_MAX; }

int main(int argc, char** argv)
{
    if (argc != 4) return fail("usage: certseg_host ARENA RAYS RESULT");
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the arena file");
    HostlaneArenaHeader AH;
    frayhip_arena::ArenaFacts F;
    if (!get(f, &AH, sizeof AH) || memcmp(AH.magic, HOSTLANE_ARENA_MAGIC, 8) != 0 || AH.factsBytes != sizeof F || !get(f, &F, sizeof F)) return fail("bad arena file");
    if (AH.nTables > (1u << 24) || AH.nMeshes != (uint64_t)F.nMeshes || AH.nTextures != (uint64_t)F.nTextures) return fail("bad arena header");
    if (F.extGeometry || F.kdMeshes || F.textured) return fail("not a scene of flag word 0");
    frayhip_arena::ArenaTable* tables = (frayhip_arena::ArenaTable*)block(AH.nTables * sizeof(frayhip_arena::ArenaTable));
    frayhip_arena::ArenaMeshTables* meshTables = (frayhip_arena::ArenaMeshTables*)block(AH.nMeshes * sizeof(frayhip_arena::ArenaMeshTables));
    int64_t* texelOffset = (int64_t*)block(AH.nTextures * sizeof(int64_t));
    if (!get(f, tables, AH.nTables * sizeof(frayhip_arena::ArenaTable)) || !get(f, meshTables, AH.nMeshes * sizeof(frayhip_arena::ArenaMeshTables)) ||
        !get(f, texelOffset, AH.nTextures * sizeof(int64_t)))
        return fail("short arena file");
    // every table into a block of exactly its size, as trace_host does: an index past a table's end is an error
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
    // frame_scene (capi.hip) with "segment_planes" and "certified_segments" on
    S.segmentPlanes = 1;
    S.certifiedSegments = S.segCertAll ? 1 : 0;

    f = fopen(argv[2], "rb");
    if (!f) return fail("cannot open the ray file");
    HostlaneRayHeader RH;
    if (!get(f, &RH, sizeof RH) || memcmp(RH.magic, HOSTLANE_RAYS_MAGIC, 8) != 0 || RH.nRays > (1u << 28) || RH.nSegs > (1u << 28)) return fail("bad ray file");
    if (fseek(f, (long)(RH.nRays * 6 * sizeof(double)), SEEK_CUR) != 0) return fail("seek");
    double* a = (double*)block(RH.nSegs * 3 * sizeof(double));
    double* b = (double*)block(RH.nSegs * 3 * sizeof(double));
    if (!get(f, a, RH.nSegs * 3 * sizeof(double)) || !get(f, b, RH.nSegs * 3 * sizeof(double))) return fail("short ray file");
    fclose(f);

    const uint64_t n = RH.nSegs;
    uint8_t* out = (uint8_t*)block(4 * n);
    uint8_t *planes = out, *gateFree = out + n, *certified = out + 2 * n, *vis = out + 3 * n;
    Cnt c;
    memset(&c, 0, sizeof c);
    for (uint64_t i = 0; i < n; i++) {
        const V3 sa = v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]), sb = v3(b[3 * i], b[3 * i + 1], b[3 * i + 2]);
        // path_shade's own call.  0 is a proof when the scene has no gates or every gate is exact, otherwise a hint
        const uint32_t gateClass = ray_gate_class(S, sa, sb - sa);
        planes[i] = segment_certified(S, sa, sb) ? 1 : 0;
        gateFree[i] = (gateClass == 0u && (S.nGates == 0 || S.gatesExact)) ? 1 : 0;
        certified[i] = segment_surely_visible(S, sa, sb, gateClass) ? 1 : 0;
        // the ray queries' own filter (query_variant.hip), as in trace_host: what fails it is visible and is not traced
        const V3 e = sb - sa;
        const double ll = e.x * e.x + e.y * e.y + e.z * e.z;
        vis[i] = (!(finite3(sa) && finite3(sb) && ll > 0.0 && ll <= DBL_MAX) || visible<0>(S, sa, sb, c)) ? 1 : 0;
    }
    FILE* o = fopen(argv[3], "wb");
    if (!o) return fail("cannot write the result file");
    const uint64_t head[4] = {n, (uint64_t)S.segCertAll, (uint64_t)S.nGates, (uint64_t)S.nSegPlanes};
    const bool ok = put(o, "FRAYCSG1", 8) && put(o, head, sizeof head) && put(o, out, 4 * n);
    if (fclose(o) != 0 || !ok) return fail("short write");
    for (uint64_t t = 0; t < AH.nTables; t++) free(where[t]);
    free(where); free(tables); free(meshTables); free(texelOffset); free(a); free(b); free(out);
    return 0;
}
