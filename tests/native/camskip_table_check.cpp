// Test harness (CPU only) of tests/test_camera_skip_host.py: the first bounce's miss records (fray_amd/csrc/dev_scene.hpp DCamSkip) as arena_build
// (fray_amd/csrc/scene_arena.hpp fill_editable) makes them of scene files.
// usage: camskip_table_check SCENE.fray ... [--update ORIGINAL.fray EDITED.fray]
// Parses each file with the product's parser, runs arena_build and prints
//   camskip <file> n=<records> nodes=<node,node,...> guards=<guard,guard,...> dirs=<nDirs,...>
// and checks the table against gatecert_make run here on each node's own triangles, taken from the description (not from the arena): a node has a record exactly
// when it is an untransformed tree-less mesh of at most FRAY_GATECERT_MAX_TRIS triangles with an index below 32 that gatecert_make accepts and fewer than
// FRAY_CAMSKIP_MAX records stand before it; the record's bytes are gatecert_make's; the records stand in node order; the table's tail is zero.
// --update: ORIGINAL's arena updated (arena_update) with EDITED's editable tables must equal EDITED's fresh arena in the record table, byte for byte, and updated
// back with ORIGINAL's it must equal ORIGINAL's fresh one.  (Both files describe one scene up to its editable part.)
// Exit code 1 with a FAIL line otherwise.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define FRAY_CERT_FN static inline
#include "host_scene.h"
#include "scene_arena.hpp"

using frayhip_arena::ArenaBuilt;

static int fail(const char* file, int node, const char* what) { printf("FAIL %s node %d: %s\n", file, node, what); return 1; }

static const DCamSkip* table(const ArenaBuilt& B) { return (const DCamSkip*)(B.host.data() + B.tables[B.F.tCamSkip].off); }

static int check(const char* file, const frayhip_scene_desc& d, const ArenaBuilt& B)
{
    const frayhip_arena::ArenaFacts& F = B.F;
    if (B.tables[F.tCamSkip].bytes != FRAY_CAMSKIP_MAX * sizeof(DCamSkip)) return fail(file, -1, "the table's size");
    const DCamSkip* R = table(B);
    static const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z3[3] = {0, 0, 0};
    int n = 0;
    for (int i = 0; i < d.n_nodes; i++) {
        const frayhip_node& N = d.nodes[i];
        bool want = d.geoms[N.geom].kind == FRAYHIP_GEOM_MESH;
        DGateTight T;
        memset(&T, 0, sizeof T);
        if (want) {
            const frayhip_mesh& m = d.meshes[d.geoms[N.geom].index];
            want = !m.has_kd && m.n_triangles > 0 && m.n_triangles <= FRAY_GATECERT_MAX_TRIS && i < 32 && n < FRAY_CAMSKIP_MAX &&
                   !memcmp(N.T.offset, Z3, sizeof Z3) && !memcmp(N.T.m, I9, sizeof I9) && !memcmp(N.T.invM, I9, sizeof I9);
            if (want) {
                std::vector<GateTri> gt;
                std::vector<double> A((size_t)3 * m.n_triangles);
                for (int t = 0; t < m.n_triangles; t++) {
                    for (int k = 0; k < 3; k++) A[3 * t + k] = m.vertices[3 * (size_t)m.triangles[t].v[0] + k];
                    gt.push_back(GateTri{&A[3 * t], m.triangles[t].AB, m.triangles[t].AC, m.triangles[t].ABcrossAC});
                }
                want = gatecert_make(T, gt.data(), m.n_triangles);
            }
        }
        const bool has = n < F.nCamSkip && R[n].node == i;
        if (want != has) return fail(file, i, want ? "an eligible node has no record" : "a node that is not eligible has a record");
        if (!has) continue;
        const DCamSkip& r = R[n++];
        if (r.nDirs != T.nDirs || r.guard != T.guard || r.Mf != T.Mf || memcmp(r.cf, T.cf, sizeof T.cf) || memcmp(r.hf, T.hf, sizeof T.hf) || memcmp(r.nf, T.nf, sizeof T.nf))
            return fail(file, i, "the record is not gatecert_make's");
        if (r.nDirs < 1 || !(r.guard > 0)) return fail(file, i, "a record without a direction or a guard");
    }
    if (n != F.nCamSkip) return fail(file, -1, "records that stand for no node, or out of node order");
    const unsigned char* tail = (const unsigned char*)(R + n);
    for (size_t b = 0; b < (FRAY_CAMSKIP_MAX - n) * sizeof(DCamSkip); b++) if (tail[b]) return fail(file, -1, "the table's tail is not zero");
    printf("camskip %s n=%d nodes=", file, n);
    for (int q = 0; q < n; q++) printf("%s%d", q ? "," : "", R[q].node);
    printf(" guards=");
    for (int q = 0; q < n; q++) printf("%s%.9g", q ? "," : "", (double)R[q].guard);
    printf(" dirs=");
    for (int q = 0; q < n; q++) printf("%s%d", q ? "," : "", R[q].nDirs);
    printf(" hmin=");
    for (int q = 0; q < n; q++) printf("%s%.9g", q ? "," : "", (double)fminf(R[q].hf[0], fminf(R[q].hf[1], R[q].hf[2])));
    printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: camskip_table_check SCENE.fray ... [--update ORIGINAL.fray EDITED.fray]\n"); return 2; }
    int a = 1;
    for (; a < argc && strcmp(argv[a], "--update") != 0; a++) {
        std::string err;
        frayhost::HostScene* hs = frayhost::parse_scene_file(argv[a], err);
        if (!hs) { fprintf(stderr, "%s: %s\n", argv[a], err.c_str()); return 2; }
        ArenaBuilt B;
        frayhip_arena::arena_build(hs->desc, B);
        if (check(argv[a], hs->desc, B)) return 1;
        delete hs;
    }
    if (a < argc) {
        if (argc - a != 3) { fprintf(stderr, "--update takes two files\n"); return 2; }
        std::string err;
        frayhost::HostScene* ho = frayhost::parse_scene_file(argv[a + 1], err);
        frayhost::HostScene* he = ho ? frayhost::parse_scene_file(argv[a + 2], err) : nullptr;
        if (!ho || !he) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
        ArenaBuilt O, E, U;
        frayhip_arena::arena_build(ho->desc, O);
        frayhip_arena::arena_build(he->desc, E);
        frayhip_arena::arena_build(ho->desc, U);
        if (check(argv[a + 1], ho->desc, O) || check(argv[a + 2], he->desc, E)) return 1;
        const size_t bytes = FRAY_CAMSKIP_MAX * sizeof(DCamSkip);
        frayhip_arena::arena_update(he->desc, U);
        if (U.F.nCamSkip != E.F.nCamSkip || memcmp(table(U), table(E), bytes)) return fail(argv[a + 2], -1, "the updated table is not the fresh one");
        if (U.host.size() != E.host.size() || memcmp(U.host.data(), E.host.data(), E.host.size())) return fail(argv[a + 2], -1, "the updated arena is not the fresh one");
        printf("updated %s n=%d\n", argv[a + 2], U.F.nCamSkip);
        frayhip_arena::arena_update(ho->desc, U);
        if (U.F.nCamSkip != O.F.nCamSkip || memcmp(table(U), table(O), bytes)) return fail(argv[a + 1], -1, "the table updated back is not the original");
        if (memcmp(U.host.data(), O.host.data(), O.host.size())) return fail(argv[a + 1], -1, "the arena updated back is not the original");
        printf("updated %s n=%d\n", argv[a + 1], U.F.nCamSkip);
        delete ho; delete he;
    }
    printf("OK\n");
    return 0;
}
