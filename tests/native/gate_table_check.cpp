// Test harness (CPU only) of tests/test_gate_table_host.py: the gate table as arena_build (fray_amd/csrc/scene_arena.hpp fill_editable) makes it of scene files.
// usage: gate_table_check SCENE.fray ...
// Parses each file with the product's parser, runs arena_build and prints one line of facts and one line of the gate table's two halves (dev_scene.hpp DGate):
//   facts <file> nGates=.. gatesExact=.. nTightGates=.. nSegNodes=.. segCertAll=..
//   tight <file> <nDirs>:<guard> per gate's tight entry ... plainDirs=<direction entries in the plain half> copies=<tight entries that are the plain entry's bytes>
// and checks every tight entry with directions against gatecert_make run here on the node's own triangles, taken from the description (not from the arena):
// box, guard and direction entries must be its record's, and every triangle's N / |N|_1 must stand among the entries, up to its sign, as FP32 rounds it.
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

static int fail(const char* file, int gate, const char* what) { printf("FAIL %s gate %d: %s\n", file, gate, what); return 1; }

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: gate_table_check SCENE.fray ...\n"); return 2; }
    for (int a = 1; a < argc; a++) {
        std::string err;
        frayhost::HostScene* hs = frayhost::parse_scene_file(argv[a], err);
        if (!hs) { fprintf(stderr, "%s: %s\n", argv[a], err.c_str()); return 2; }
        const frayhip_scene_desc& d = hs->desc;
        ArenaBuilt B;
        frayhip_arena::arena_build(d, B);
        const frayhip_arena::ArenaFacts& F = B.F;
        printf("facts %s nGates=%d gatesExact=%d nTightGates=%d nSegNodes=%d segCertAll=%d\n", argv[a], F.nGates, F.gatesExact, F.nTightGates, F.nSegNodes, F.segCertAll);
        const DGate* G = (const DGate*)(B.host.data() + B.tables[F.tGates].off);
        const DNode* nodes = (const DNode*)(B.host.data() + B.tables[F.tNodes].off);
        // the gates stand in node order: the nodes of tree-less meshes of FRAY_GATE_MIN_TRIS triangles or more (these scenes have no CSG nodes)
        std::vector<int> gateNode;
        for (int i = 0; i < d.n_nodes && (int)gateNode.size() < FRAY_MAX_GATES; i++)
            if (nodes[i].tlTris >= FRAY_GATE_MIN_TRIS) gateNode.push_back(i);
        if ((int)gateNode.size() != F.nGates) return fail(argv[a], -1, "the gates are not the tree-less meshes in node order");
        printf("tight %s", argv[a]);
        int plainDirs = 0, copies = 0, withDirs = 0;
        for (int q = 0; q < F.nGates; q++) {
            const DGate& P = G[q];
            const DGate& T = G[q + FRAY_MAX_GATES];
            printf(" %d:%.9g", T.nDirs, (double)T.guard);
            plainDirs += P.nDirs;
            copies += T.nDirs == 0 && memcmp(&P, &T, sizeof(DGate)) == 0;
            withDirs += T.nDirs != 0;
        }
        printf(" plainDirs=%d copies=%d\n", plainDirs, copies);
        if (withDirs != F.nTightGates || withDirs + copies != F.nGates) return fail(argv[a], -1, "an entry is neither a tight record nor the plain entry again");
        for (int q = 0; q < F.nGates; q++) {
            const DGate& T = G[q + FRAY_MAX_GATES];
            const frayhip_mesh& m = d.meshes[d.geoms[d.nodes[gateNode[q]].geom].index];
            std::vector<GateTri> gt;
            std::vector<double> A((size_t)3 * m.n_triangles);
            for (int t = 0; t < m.n_triangles; t++) {
                for (int k = 0; k < 3; k++) A[3 * t + k] = m.vertices[3 * (size_t)m.triangles[t].v[0] + k];
                gt.push_back(GateTri{&A[3 * t], m.triangles[t].AB, m.triangles[t].AC, m.triangles[t].ABcrossAC});
            }
            DGateTight R;
            const bool made = m.n_triangles <= FRAY_GATECERT_MAX_TRIS && G[q].exact && gatecert_make(R, gt.data(), m.n_triangles);
            if (made != (T.nDirs != 0)) return fail(argv[a], q, "eligibility differs from gatecert_make on the mesh's triangles");
            if (!made) continue;
            if (T.nDirs != R.nDirs || T.guard != R.guard || T.Mf != R.Mf || memcmp(T.cf, R.cf, sizeof R.cf) || memcmp(T.hf, R.hf, sizeof R.hf) || memcmp(T.nf, R.nf, sizeof R.nf))
                return fail(argv[a], q, "the tight entry is not gatecert_make's record");
            if (!T.exact) return fail(argv[a], q, "a tight entry that is not exact");
            for (int t = 0; t < m.n_triangles; t++) {
                const double* N = m.triangles[t].ABcrossAC;
                const double n1 = fabs(N[0]) + fabs(N[1]) + fabs(N[2]);
                bool found = false;
                for (int j = 0; j < T.nDirs && !found; j++) {
                    double same = 0, opp = 0;
                    for (int k = 0; k < 3; k++) { same = fmax(same, fabs(T.nf[j][k] - N[k] / n1)); opp = fmax(opp, fabs(T.nf[j][k] + N[k] / n1)); }
                    found = fmin(same, opp) <= 0x1p-23;          // the entry is the direction rounded to FP32
                }
                if (!found) return fail(argv[a], q, "a triangle's direction is missing from the entries");
            }
        }
        delete hs;
    }
    printf("OK\n");
    return 0;
}
