// The three files of the host lane (tests/test_trace_host.py), native byte order, no padding between the parts.
//
// arena file (arena_dump -> trace_host):
//   HostlaneArenaHeader, ArenaFacts, ArenaTable[nTables], ArenaMeshTables[nMeshes], int64 texelOffset[nTextures], the arena's bytes
// ray file (the test -> trace_host):
//   HostlaneRayHeader, double o[3 nRays], d[3 nRays], a[3 nSegs], b[3 nSegs]
// result file (trace_host -> the test):
//   HostlaneResultHeader
//   int32 id[nRays], double rec[9 nRays]                  closest_hit<w> and k_query_closest<w, true>'s record
//   int32 idC[nRays], double recC[9 nRays]                the same from w | 1
//   uint64 cntClosest[11]                                 w | 1's counters summed over the rays (Cnt's order, envelope last)
//   uint8 vis[nSegs], visC[nSegs]                         visible<w>, visible<w | 1>
//   uint64 cntVisible[11]
//   uint8 visP[nSegs], uint32 skip[nSegs]                 words 0 and 8: the SEGP copy and the word of nodes it skipped (zeros for the others)
#pragma once
#include <stdint.h>

#define HOSTLANE_ARENA_MAGIC "FRAYARN1"
#define HOSTLANE_RAYS_MAGIC "FRAYRAY1"
#define HOSTLANE_RESULT_MAGIC "FRAYRES1"

struct HostlaneArenaHeader { char magic[8]; uint64_t nTables, nMeshes, nTextures, arenaBytes, factsBytes; };
struct HostlaneRayHeader { char magic[8]; uint64_t nRays, nSegs; };
struct HostlaneResultHeader { char magic[8]; uint64_t word, nRays, nSegs, segp; };
