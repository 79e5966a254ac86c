// Test harness (CPU only), first half of the host lane (tests/test_trace_host.py): parses .fray files with the product's parser, runs
// arena_build (fray_amd/csrc/scene_arena.hpp) and writes the UNPLACED arena, its table list and the scene facts to a file each, for trace_host.
// usage: arena_dump [--env-unloaded] SCENE.fray OUT [[--env-unloaded] SCENE.fray OUT ...]
//   --env-unloaded: the next scene's environment map counts as not loaded (the reference fixtures made without an EXR reader, tests/test_oracle_vs_ref.py)
// Built with AddressSanitizer + UndefinedBehaviorSanitizer: the builder's own indexing is checked on the way.
#include <cstdio>
#include <cstring>
#include <string>

#define FRAY_CERT_FN static inline
#include "host_scene.h"
#include "scene_arena.hpp"
#include "hostlane_format.h"

static bool put(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: arena_dump [--env-unloaded] SCENE.fray OUT ...\n"); return 2; }
    for (int i = 1; i < argc; i += 2) {
        const bool envUnloaded = !strcmp(argv[i], "--env-unloaded");
        if (envUnloaded) i++;
        if (i + 1 >= argc) { fprintf(stderr, "arena_dump: a scene without an output file\n"); return 2; }
        std::string err;
        frayhost::HostScene* hs = frayhost::parse_scene_file(argv[i], err);
        if (!hs) { fprintf(stderr, "arena_dump: %s: %s\n", argv[i], err.c_str()); return 1; }
        if (envUnloaded) hs->desc.environment.loaded = 0;
        frayhip_arena::ArenaBuilt B;
        frayhip_arena::arena_build(hs->desc, B);
        HostlaneArenaHeader H;
        memset(&H, 0, sizeof H);
        memcpy(H.magic, HOSTLANE_ARENA_MAGIC, 8);
        H.nTables = B.tables.size(); H.nMeshes = B.meshTables.size(); H.nTextures = B.texelOffset.size(); H.arenaBytes = B.host.size();
        H.factsBytes = sizeof(frayhip_arena::ArenaFacts);
        FILE* f = fopen(argv[i + 1], "wb");
        if (!f) { fprintf(stderr, "arena_dump: cannot write %s\n", argv[i + 1]); return 1; }
        const bool ok = put(f, &H, sizeof H) && put(f, &B.F, sizeof B.F) && put(f, B.tables.data(), B.tables.size() * sizeof(frayhip_arena::ArenaTable)) &&
                        put(f, B.meshTables.data(), B.meshTables.size() * sizeof(frayhip_arena::ArenaMeshTables)) &&
                        put(f, B.texelOffset.data(), B.texelOffset.size() * sizeof(int64_t)) && put(f, B.host.data(), B.host.size());
        if (fclose(f) != 0 || !ok) { fprintf(stderr, "arena_dump: short write to %s\n", argv[i + 1]); return 1; }
        const frayhip_arena::ArenaFacts& F = B.F;
        printf("%s: flag word %d, %zu tables, %zu bytes, %d nodes, %d segment-plane nodes\n", argv[i], F.extGeometry ? 2 : F.kdMeshes ? 4 : F.textured ? 8 : 0,
               B.tables.size(), B.host.size(), F.nNodes, F.nSegNodes);
        delete hs;
    }
    return 0;
}
