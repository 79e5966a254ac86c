// "This ray surely misses this mesh": a certificate under which NO triangle of an untransformed mesh without a KD-tree is accepted by
// Mesh::intersectTriangle (mesh.cpp:102-141, with Triangle::intersectFast, triangle.cpp:66-94) -- not in real arithmetic only, but as the reference's
// own code computes it, and as this project's two copies of it do (dev_trace.hpp tri_test under node_intersect / closest_hit / visible: the exact copy
// and the fp_contract one, with fused products and the two-ulp reciprocal of dev_math.hpp).  dev_misscert.hpp proves the same for the mesh's BOX
// (BBox::testIntersect guards the triangle loop); but the box of a mesh loaded from an OBJ file contains the loader's dummy vertex (0, 0, 0), and the
// two blocks of cornell_box, whose gates these are, fill a fraction of theirs.  Here the box is the one of the triangles themselves, and since no box
// test of the reference stands behind it the proof has to speak about every triangle test.
//
// Notation.  A triangle record holds A, AB, AC and N (= AB x AC as the loader rounded it).  The REAL triangle is the one with the corners A, A + AB,
// A + AC in real arithmetic, N* = AB x AC its real normal, n1 = |N|_1.  The ray is the queue's: start s (FP64, used as it is: an untransformed node's
// local start is s bit for bit) and direction q (FP64; a unit vector or an unnormalised segment b - a); dh = q / |q|_2 in real arithmetic.  The code
// under test normalises q once, twice or (visible()) three times: its direction d has d_k = dh_k (1 + e_k), |e_k| <= 16u, u = 2^-53.  With H* = s - A:
//     Dcr* = -N* . dh,    gamma* = N* . H* / Dcr*,    l2* = (H* x AC) . (-dh) / Dcr*,    l3* = (AB x H*) . (-dh) / Dcr*,    l1* = 1 - l2* - l3*
// are the parameter and the barycentrics of P* = s + gamma* dh = A + l2* AB + l3* AC, the point where the ray's LINE crosses the triangle's plane.
// The mesh's constants, all made by gatecert_make below (rounded towards the safe side):
//     box      [lo, hi] of all corners, centre c, half extents h, M = max_k (|c_k| + h_k);    R = |s|_inf + M >= |H*|_inf
//     E        max |AB|_inf, |AC|_inf over the triangles;      n1min = min n1;      nu = E^2 / n1min          (nu is large for a sliver)
//     kappa    0.98 min over the triangles of  Lmin / (2 Lmax^2),  Lmin / Lmax the shortest / longest edge (2-norm)
//     G        the guard threshold, below.
//
// The certificate holds when
//   (B) ray_surely_misses_box_f32 (dev_misscert.hpp) holds for the box [lo, hi]: by its proof the real line through s along q passes the box at a
//       distance (inf-norm) of more than m = 1e-5 + 2^-22 R (its condition 2), or the box lies behind the start by more than m in some coordinate k
//       in which the ray does not advance (condition 1);  write m' = m / 2 >= max(0.5e-5, 2^-23 R);
//   (G) for every normal direction nf of the mesh (N / n1 of its triangles; opposite and equal directions share an entry; at most FRAY_GATE_MAX_DIRS):
//       |fl32(nf . q)| > Gf |q~|_1,  Gf = G + 2^-18 -- the FP32 evaluation errs by less than 2^-20 |q|_1 and entries that share a direction differ by at
//       most 2^-30 -- so that |Dcr*| >= G n1 for every triangle;
//   (R) 2^-40 <= |q~|_1 <= 2^40, |s~|_inf < 1e9 and no coordinate of s~ is a NaN; M < 2^24: every normalisation, product and reciprocal below is finite
//       and normal.  A NaN or an infinity in s or q fails (R): its comparisons are false for them.
//
// Proof.  Step 1: P* lies at a distance of more than m' from the box, or gamma* <= -m' (1 - 2^-40).
//   Under condition 2 the whole line is farther than m from the box.  Under condition 1, say s_k > hi_k + m and q_k >= 0: if gamma* >= 0 then
//   P*_k >= s_k; if gamma* < 0 and P*_k <= hi_k + m' then -gamma* dh_k > m', and dh_k <= 1.  (q_k is tested as fl32(q_k), which is 0 for |q_k| < 2^-150
//   whatever its sign; with |q|_1 >= 2^-40 such a ray needs a parameter beyond 2^100 to advance m' in coordinate k and is by then 2^60 away from
//   everything: P* is far from the box.)
// Step 2: a point of the plane at a distance r from the real triangle has some barycentric l_j* <= -r Lmin / (2 Lmax^2) = -delta,  delta >= m' kappa.
//   Let Q be the triangle's point nearest to P*.  If Q is inside an edge, P* is r beyond that edge's line and l_j* = -r / h_j, h_j the height onto it.
//   If Q is a corner of angle theta, P* lies in the corner's normal cone, of angle pi - theta, and is at least r sin(theta / 2) beyond the line of one
//   of the two edges.  sin(theta / 2) >= sin(theta) / 2 >= Area / Lmax^2 and h_j <= 2 Area / Lmin: the area cancels.
// Step 3: the computed values.  H~ = fl(s - A); the numerators M2~, M3~ of l2, l3 are each three 2x2 determinants and a dot product of terms below
//   2 R E |d_k|; with the 16u of d and the u of H~ they lie within dM = 128u R E of M2*, M3* (the fused copy's errors are smaller).  N differs from
//   N* by at most 2^-46 E^2 per component (gatecert_make checks 2^-48 against its own cross product), so Dcr~ = fl(N . -d) lies within
//   (256 nu + 24) u n1 of Dcr*, and sg~ = fl(N . H~) within (384 nu + 8) u n1 R of sg* = N* . H*.  With (G), rhoD = (256 nu + 24) u / G bounds the
//   relative error of Dcr~: it has the sign of Dcr* and r~ = fl(1 / Dcr~) is finite (relative error 4u in either copy).  So
//       l_j~ = l_j* (1 + rho_j) + a_j,     |rho_j| <= rho = 2 rhoD + 8u,     |a_j| <= a = 1.01 dM / (G n1)                       (j = 2, 3).
//   * gamma* <= -0.99 m':  |sg*| = |gamma*| |Dcr*| >= 0.99 m' G n1 > 2 (384 nu + 8) u n1 R  by (G3) below, so sg~ has the sign of sg*, gamma~ =
//     fl(sg~ r~) < 0 (|gamma~| >= 0.2 m' G: no underflow) and the triangle is rejected at `gamma < 0`.
//   * l2* <= -delta (or l3*):  l2~ <= -delta (1 - rho) + a < -delta / 2 by (G1): rejected at `l2 < 0`.
//   * l1* <= -delta and l2~ >= 0, l3~ >= 0 (else rejected):  then l2*, l3* >= -1.01 a, so |l2*| + |l3*| <= l2* + l3* + 4.1 a, and
//         l2~ + l3~ >= (l2* + l3*)(1 - rho) - 2.1 a >= (1 + delta)(1 - rho) - 2.1 a >= 1 + delta / 2 - ...  > 1 + delta / 4
//     by (G1) a <= delta / 8 and (G2) rho <= delta / 4 -- more than 2^-42 above 1, so the rounded sum exceeds 1 and l1~ = fl(1 - sum) < 0: rejected.
//   The thresholds, with m' >= 2^-23 R and delta >= dmin = kappa max(0.5e-5, 2^-23 M):
//       (G1)  a <= delta / 8      <=   G >= 1040 u R E / (n1min m' kappa)   <=   G >= 1040 2^-30 E / (n1min kappa)
//       (G2)  rho <= delta / 4    <=   G >= 16 (256 nu + 24) u / dmin       (dmin >= 2^-40 required, so that 8u <= dmin / 32)
//       (G3)                           G >= 2.1 (384 nu + 8) 2^-30
//   G is TWICE the largest of the three.  A mesh is eligible when Gf <= 2^-6 and nu <= 2^12 (cornell_box's blocks: nu = 4, G = 4e-5).
//   |Dcr~| < 1e-12 is rejected by the code itself; the culling test, `gamma > best`, `l2 > 1` and `l3 > 1` only reject more; no NaN arises by (R).
//   So every triangle of the mesh is rejected whatever `best` is, and the mesh reports no intersection -- whether its reference box test passes or not.
// tests/native/gatecert_check.cpp runs the function on the host against the triangle test and the mesh loop restated from the reference, in both
// arithmetics, over random and adversarial rays; built with FRAY_GATECERT_SCALE = 0 (no margin, no guard) the same harness finds contradictions.
#pragma once
#include <stdint.h>
#include "dev_misscert.hpp"
#ifndef FRAY_GATECERT_SCALE
#define FRAY_GATECERT_SCALE 1      // 0: the harness's second build -- no margin in the box part (with FRAY_MISSCERT_SCALE = 0), no guard
#endif
#define FRAY_GATE_MAX_DIRS 6       // normal directions per tight gate (a box has three; cornell_box's blocks, whose sides are not quite parallel, five)
#define FRAY_GATECERT_MAX_TRIS 32  // triangles gatecert_make looks at; a mesh with more gets no tight record
#define FRAY_GATECERT_MAX_COORD 0x1p24
#define FRAY_GATECERT_MAX_NU 0x1p12
#define FRAY_GATECERT_MAX_GUARD 0x1p-6f

// The tight record of a gate (what the tight half of the gate table takes from it, dev_scene.hpp DGate): the FP32 box of the mesh's own triangles in ray_surely_misses_box_f32's form, the guard
// threshold Gf and the normal directions nf = N / |N|_1.  tight = 0: the mesh is not eligible, everything else is zero.
struct DGateTight { float cf[3], hf[3]; float Mf, guard; float nf[FRAY_GATE_MAX_DIRS][3]; int32_t nDirs, tight; };      // 112 B

// (G) for one direction entry; gd = Gf |q~|_1.  (R)'s bounds on the ray are gate_ray_range (osum = ox + oy + oz).
FRAY_CERT_FN bool gate_dir_guard(float nx, float ny, float nz, float dx, float dy, float dz, float gd)
{
    return __builtin_fabsf(__builtin_fmaf(nz, dz, __builtin_fmaf(ny, dy, nx * dx))) > gd;
}
// (a NaN coordinate of the start is dropped by fmaxf from omax but kept by the sum; with one, H~ and every value after it is a NaN, and a NaN passes `!(x < 0)`)
FRAY_CERT_FN bool gate_ray_range(float dsum, float omax, float osum) { return dsum >= 0x1p-40f && dsum <= 0x1p40f && omax < 1e9f && osum == osum; }

// (G) for one record: DGateTight, or a tight entry of the gate table (DGate, on the device through the constant address space).  The direction alone.
template <class GT>
FRAY_CERT_FN bool gate_guard_f32(const GT& T, float dx, float dy, float dz, float dsum)
{
    bool ok = true;
    const float gd = (FRAY_GATECERT_SCALE ? T.guard : 0.0f) * dsum;
    for (int j = 0; j < T.nDirs; j++) ok = ok & gate_dir_guard(T.nf[j][0], T.nf[j][1], T.nf[j][2], dx, dy, dz, gd);
    return ok;
}
// The whole certificate for one record (the harness calls this form; ray_gate_class evaluates the same three parts, the guards of all gates first):
// (o, d) the queue's ray converted to FP32, omax = |o~|_inf, dsum = |d~|_1.
template <class GT>
FRAY_CERT_FN bool ray_surely_misses_mesh_f32(const GT& T, float ox, float oy, float oz, float dx, float dy, float dz, float omax, float dsum)
{
    return ray_surely_misses_box_f32(T.cf[0], T.cf[1], T.cf[2], T.hf[0], T.hf[1], T.hf[2], T.Mf, ox, oy, oz, dx, dy, dz, omax, dsum) &
           gate_guard_f32(T, dx, dy, dz, dsum) & gate_ray_range(dsum, omax, ox + oy + oz);
}

// ---- host side (scene_arena.hpp fill_editable, the harness) ---------------------------------------------------------------------------------
#include <math.h>
struct GateTri { const double *A, *AB, *AC, *N; };      // one triangle record's four vectors (DTri)

// Decides eligibility and makes the record.  Returns false, with `o` zeroed, when the mesh gets none: a non-finite or too large coordinate, a
// degenerate edge, a stored normal that is not its edges' cross product, a sliver (nu, or a guard above FRAY_GATECERT_MAX_GUARD), more than
// FRAY_GATE_MAX_DIRS normal directions or more than FRAY_GATECERT_MAX_TRIS triangles.
static inline bool gatecert_make(DGateTight& o, const GateTri* tris, int n)
{
    DGateTight z;
    for (int k = 0; k < 3; k++) z.cf[k] = z.hf[k] = 0;
    z.Mf = z.guard = 0; z.nDirs = 0; z.tight = 0;
    for (int j = 0; j < FRAY_GATE_MAX_DIRS; j++) z.nf[j][0] = z.nf[j][1] = z.nf[j][2] = 0;
    o = z;
    if (n <= 0 || n > FRAY_GATECERT_MAX_TRIS) return false;
    const double u = 0x1p-53;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    double E = 0, n1min = 1e300, kappa = 1e300, Mabs = 0;
    double dirs[FRAY_GATE_MAX_DIRS][3];
    int nDirs = 0;
    for (int t = 0; t < n; t++) {
        const double *A = tris[t].A, *AB = tris[t].AB, *AC = tris[t].AC, *N = tris[t].N;
        double n1 = 0, l0 = 0, l1 = 0, l2 = 0;
        for (int k = 0; k < 3; k++) {
            const double v[3] = {A[k], A[k] + AB[k], A[k] + AC[k]};
            for (int c = 0; c < 3; c++) {
                if (!(fabs(v[c]) <= FRAY_GATECERT_MAX_COORD)) return false;          // (false on NaN)
                lo[k] = v[c] < lo[k] ? v[c] : lo[k]; hi[k] = v[c] > hi[k] ? v[c] : hi[k];
                Mabs = fabs(v[c]) > Mabs ? fabs(v[c]) : Mabs;
            }
            if (!(fabs(AB[k]) <= 2 * FRAY_GATECERT_MAX_COORD) || !(fabs(AC[k]) <= 2 * FRAY_GATECERT_MAX_COORD) || !(N[k] == N[k])) return false;
            E = fabs(AB[k]) > E ? fabs(AB[k]) : E; E = fabs(AC[k]) > E ? fabs(AC[k]) : E;
            const int a = (k + 1) % 3, b = (k + 2) % 3;
            const double p = AB[a] * AC[b], q = AB[b] * AC[a];
            if (!(fabs(N[k] - (p - q)) <= 0x1p-48 * (fabs(p) + fabs(q)))) return false;      // N is AB x AC as some compiler rounded it
            n1 += fabs(N[k]);
            const double e2 = AC[k] - AB[k];
            l0 += AB[k] * AB[k]; l1 += AC[k] * AC[k]; l2 += e2 * e2;
        }
        const double lmin2 = fmin(l0, fmin(l1, l2)), lmax2 = fmax(l0, fmax(l1, l2));
        if (!(lmin2 > 0) || !(n1 > 0)) return false;
        kappa = fmin(kappa, 0.98 * sqrt(lmin2) / (2 * lmax2));
        n1min = fmin(n1min, n1);
        // the direction entry: N / n1, shared with an equal or opposite one
        const double dn[3] = {N[0] / n1, N[1] / n1, N[2] / n1};
        int j = 0;
        for (; j < nDirs; j++) {
            double same = 0, opp = 0;
            for (int k = 0; k < 3; k++) { same = fmax(same, fabs(dirs[j][k] - dn[k])); opp = fmax(opp, fabs(dirs[j][k] + dn[k])); }
            if (fmin(same, opp) <= 0x1p-30) break;
        }
        if (j == nDirs) {
            if (nDirs == FRAY_GATE_MAX_DIRS) return false;
            for (int k = 0; k < 3; k++) dirs[nDirs][k] = dn[k];
            nDirs++;
        }
    }
    const double nu = E * E / n1min * (1 + 0x1p-40);
    if (!(nu <= FRAY_GATECERT_MAX_NU)) return false;
    DGateTight g = z;
    double M = 0;
    for (int k = 0; k < 3; k++) {
        const double c = 0.5 * (lo[k] + hi[k]), half = fmax(hi[k] - c, c - lo[k]);
        g.cf[k] = (float)c;
        // the corners as computed (A + AB rounds by u Mabs), dev_misscert.hpp's constant margin, the centre's rounding -- rounded up
        g.hf[k] = nextafterf((float)(half * (1.0 + 1e-12) + 0x1p-48 * Mabs + FRAY_GATECERT_SCALE * 1e-5 + fabs(c - (double)g.cf[k])), INFINITY);
        g.Mf = fmaxf(g.Mf, nextafterf(fabsf(g.cf[k]) + g.hf[k], INFINITY));
        M = fmax(M, fabs(c) + half);
    }
    if (!(g.Mf < 0x1p24f)) return false;
    const double dmin = kappa * fmax(0.5e-5, 0x1p-23 * M);
    if (!(dmin >= 0x1p-40)) return false;
    const double G1 = 1040 * 0x1p-30 * E / (n1min * kappa), G2 = 16 * (256 * nu + 24) * u / dmin, G3 = 2.1 * (384 * nu + 8) * 0x1p-30;
    const double G = 2 * fmax(G1, fmax(G2, G3));
    if (!(G <= 1.0)) return false;
    g.guard = nextafterf((float)G + 0x1p-18f, INFINITY);
    if (!(g.guard <= FRAY_GATECERT_MAX_GUARD)) return false;
    for (int j = 0; j < nDirs; j++) for (int k = 0; k < 3; k++) g.nf[j][k] = (float)dirs[j][k];
    g.nDirs = nDirs; g.tight = 1;
    o = g;
    return true;
}
