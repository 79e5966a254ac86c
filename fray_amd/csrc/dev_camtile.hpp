// "No camera ray of this 8x8 pixel tile hits this mesh": dev_gatecert.hpp's certificate decided ONCE for all the rays a mono pinhole frame can send through a
// tile, whatever their jitter and their sample index, from the tile's four corner directions (frayhip_scene_camera_tiles; kernels.hpp k_pt_bounce<0, false, true>
// reads the answer from a per-frame table, k_cam_tiles fills it).  dev_trace.hpp camera_skip_nodes asks the same seven questions of every lane's
// ray at every sample index: about 400 vector instructions per wave iteration for an answer that is a property of the tile.
//
// Setting.  A mono pinhole frame (no `dof`, no stereo): screen_ray (kernels.hpp) gives every ray the start o = C.pos, bit for bit, and the direction
//     d = normalized(q^),    q^ = fl(tl + ex fl(x / w) + ey fl(y / h)),    ex = fl(tr - tl),  ey = fl(bl - tl)      (FP64, no contraction)
// where x = (double)((float)px + jx), jx in [0, 1): the float sum may round up to px + 1, so x lies in [px, px + 1], and for the pixels of the tile with the
// origin (x0, y0) in [x0, x0 + 8]; y likewise.  q*(x, y) = tl + ex x / w + ey y / h in real arithmetic -- with ex, ey the FP64 numbers above -- is AFFINE in
// (x, y); the rectangle [x0, x0 + 8] x [y0, y0 + 8] has four corners c, and q_c is q^ evaluated at corner c by cam_tile_rays below, with screen_ray's own expression.
// Q = max_c |q_c|_1,  S2 = 2 (|tl|_inf + |ex|_inf + |ey|_inf),  u = 2^-53.
//
// The certificate for a record (cf, hf, Mf, guard Gf, directions nf_j: DCamSkip / DGateTight), with p = fl(o - cf), and H = hf + eta, eta and `slack` exactly as in
// ray_surely_misses_box_f32 (dev_misscert.hpp: slack = 2^-19 (|o|_inf + |p|_inf), eta = 2^-21 (|o|_inf + Mf) + slack), all evaluated in FP64:
//   (R_t) w, h > 0, x0 + 8 <= 2 w, y0 + 8 <= 2 h;  2^-40 <= |q_c|_1 <= 2^40 and 64 |q_c|_1 >= S2 at every corner;  for some coordinate k the four q_{c,k} have one
//         sign and min_c |q_{c,k}| >= 2^-8 Q;  |o_k| < 1e9 and no coordinate of o is a NaN  (gate_ray_range's bounds, on o and on the corners).
//   (G_t) for every direction entry nf_j: the four nf_j . q_c have one sign and min_c |nf_j . q_c| > Gf (1 + 2^-20) Q.
//   (B_t) (1) for some k:  p_k > H_k and q_{c,k} >= 0 at all four corners,  or  p_k < -H_k and q_{c,k} <= 0 at all four;  or
//         (2) for some axis k with the other two (u, v): the four L_c = q_{c,u} p_v - q_{c,v} p_u have one sign and
//             min_c |L_c| > max_c (|q_{c,v}| H_u + |q_{c,u}| H_v) (1 + 2^-20) + slack Q + 2^-40 Q (H_u + H_v).
//
// Claim: under (R_t), (G_t), (B_t) every ray of the tile satisfies the two real facts dev_gatecert.hpp's proof takes from its conditions (B) and (G) -- the real
// line from o along d passes the record's box at more than m = 1e-5 + 2^-22 R (or the box lies behind the start, Step 1), and |nf . dh| > G for every direction
// entry -- and (R).  Steps 1 to 3 of that proof then reject every triangle of the mesh for that ray, in both arithmetics.
//
// Proof.  Rounding.  By (R_t) |fl(x / w)| <= 2 (1 + u) and likewise for y: each product errs by at most 2u of a term below 2 |ex|_inf (2 |ey|_inf), each of the two
//   additions by u of a partial sum below S2: |q^ - q*|_inf <= 4u S2 <= 2^-45 |q_c|_1 for every corner, hence <= 2^-45 Q.  The same holds for q_c against
//   q*_c = q*(corner).  normalized() multiplies by one rounded reciprocal of a rounded square root: d_k = dhat_k (1 + e_k), |e_k| <= 4u, dhat = q^ / |q^|_2.
//   All conditions of (B) and (G) are homogeneous in the direction, so it suffices to show them for q' = |q^|_2 d, and |q' - q*|_inf <= 2^-45 Q + 4u |q^|_inf
//   <= 2^-44 Q =: delta.
//   Size.  |.|_1 is convex: |q*|_1 <= max_c |q*_c|_1 <= Q (1 + 2^-44) on the whole rectangle.  q*_k of (R_t)'s coordinate is affine and lies between its corner
//   values, which have one sign: |q'|_1 >= |q*_k| - delta >= 2^-9 Q >= 2^-49.  So q^ is finite, normal and far from underflow, d is a unit vector within 4u
//   and gatecert's (R) holds for the ray (o, d) as camera_skip_nodes would test it (|d~|_1 in [1, 2], the bounds on o are tested on o itself).
//   (G).  f(q) = nf_j . q is affine, so f(q*) lies between the four f(q*_c).  The computed corner values differ from f(q*_c) by less than 2^-43 Q (|nf_j|_1 <=
//   1 + 2^-20; three products and two sums of terms below Q; the corner's own 2^-45 Q).  They have one sign and exceed Gf Q >= 2^-18 Q in magnitude, so the real
//   ones have that sign too and |f(q')| >= min_c |f(q*_c)| - 1.01 delta > (Gf (1 + 2^-20) - 2^-42) Q > (Gf - 2^-19) |q'|_1 = (G + 2^-19) |q'|_1.  The per-ray form
//   reaches G + 2^-18 - 2^-20 in the same place (its FP32 evaluation errs by 2^-20 |q|_1); the 2^-30 between entries that share a direction is covered alike.
//   (B)(2).  L(q) = q_u p_v - q_v p_u is affine in q, so L(q*) lies between the L(q*_c), and those lie within (6u + 2^-44) Q |p|_inf of the computed L_c, which
//   have one sign: |L(q')| >= min_c |L_c| - 2^-42 Q |p|_inf.  r(q) = |q_v| H_u + |q_u| H_v is convex: r(q') <= max_c r(q*_c) + delta (H_u + H_v) <=
//   max_c r_c (1 + 4u) + 2^-43 Q (H_u + H_v), r_c the computed ones.  The FP64 form (ray_surely_misses_box; for a direction that is no unit vector its
//   absolute term is multiplied by |q'|_2 <= |q'|_1) asks |L(q')| > r64(q') (1 + 2^-40) + 2^-40 |p|_inf |q'|_1, where r64 <= r because H64 = hf + 2^-22 (|o|_inf + M)
//   <= H.  The condition tested gives |L(q')| > max_c r_c (1 + 2^-20) + slack Q + 2^-40 Q (H_u + H_v) - 2^-42 Q |p|_inf: the factor 2^-20 covers 2^-40 + 4u, the
//   third term the 2^-43 Q (H_u + H_v) eight times (it is this form's own: the per-ray form has no delta), and slack Q >= 2^-19 Q |p|_inf both the 2^-40 |p|_inf |q'|_1
//   and the 2^-42 Q |p|_inf, 2^20 times.  So the real line misses the box widened by eta64, i.e. passes the true box at more than m.
//   (B)(1).  p_k > H_k (a statement about the start alone, with the per-ray form's margin and 2^29 u of room for the one rounding of p).  q*_k is affine and
//   lies between corner values that are >= -2^-45 Q, so q'_k >= -2^-43 Q and dh_k >= -2^-43 Q / |q'|_2 >= -2^-33 (|q'|_2 >= |q'|_1 / 2 >= 2^-10 Q).  Where q'_k >= 0
//   this is the per-ray form's condition 1.  Otherwise Step 1's remark applies with 2^-33 in the place of 2^-110: to advance m' in coordinate k the line needs a
//   parameter beyond 2^33 m', and m' >= max(0.5e-5, 2^-23 R): the point is then more than 2^33 m' - 2 R > m' away from everything within R of the start, the
//   box included -- P* is far from the box or gamma* < 0.
//   The margins kept from the FP32 form are 2^29 times an FP64 rounding; what they have to cover here -- this evaluation's own rounding, a few u, and delta, the gap
//   between the computed q^ of any ray and the affine q*, 2^-44 relative to Q -- is 2^9 u.
//
// Asked nodes.  (G_t) fails for a tile that holds a direction parallel to a face -- the rows of tiles at the horizon for a floor, the columns beside the image's
// centre for a side wall -- although a sample's 64 rays hardly ever come within the guard's 1e-5 of it.  The two real facts are independent: where (R_t) and (B_t)
// hold for the tile and (G_t) does not, the table says so in a second word (`ask`, bit `node`), and the wave evaluates the per-ray form's (G) and (R) -- FP32, on
// its own rays, dev_gatecert.hpp as it stands -- for those records only (dev_trace.hpp camera_guard_nodes).  A node it then skips has (B) by the tile's proof above
// and (G), (R) by the per-ray form's own: both facts hold for every ray of the wave.  On the headline frame those are the tile row and the two tile columns through the image centre (of 135 and 240) and a few tiles along the blocks' faces: about two tiles in a hundred, counted from the frame's geometry, not measured.
//
// The per-ray form certifies a wave when each of its 64 rays passes; this one when the corners do.  On the headline frame a float64 model of both (32 400 tiles, 8
// jitter sets) gives 5.639 against 5.653 skipped nodes per wave, and no (tile, sample, record) the corner form certifies and the per-ray form does not.
// tests/native/camtile_check.cpp runs this header on the host against the mesh loop restated from the reference, in both arithmetics; built with
// FRAY_CAMTILE_SCALE = 0 (and the other two scales 0: no margin, no guard) the same harness finds contradictions.
#pragma once
#include <stdint.h>
#include "frayhip.h"
#include "dev_gatecert.hpp"
#ifndef FRAY_CAMTILE_SCALE
#define FRAY_CAMTILE_SCALE 1       // 0: the harness's second build -- no margins, no guard
#endif

// One entry of the frame's tile table, per 64-item tile in item order: the nodes no camera ray of the tile can hit (bit `node`; zero while the switch is off, for
// a `dof` camera and without miss records) and the tile's pixel origin -- item_pixel of the tile's item 0.
struct DCamTile { uint32_t skip; uint16_t x0, y0; };      // 8 B
#define FRAY_CAMTILE_MAX_COORD 65536      // a frame whose bucket grid reaches beyond gets no table (uint16 origins)

// ---- work item -> pixel ------------------------------------------------------------------------
// Inside a 48x48 bucket the items run over 8x8 pixel tiles (6x6 of them), so the 64 lanes of a wave
// hold a square of neighbouring pixels: their camera rays walk the same part of a KD-tree.  Every
// (pixel, sample) is independent, so the order has no effect on the picture.
// (kernels.hpp item_pixel is this function; the host harness of the tile table compiles it too.)
template <class FR>
FRAY_CERT_FN bool frame_item_pixel(const FR& F, int item, int& x, int& y)
{
    int k = item / 2304, local = item - k * 2304;
    int b = F.bucketFirst + k * F.bucketStride;
    int by = b / F.BW, bx = (b - by * F.BW + FRAYHIP_BUCKET_SKEW * by) % F.BW;      // frayhip_bucket_xy (include/frayhip.h)
    int tile = local >> 6, in = local & 63;
    x = bx * 48 + (tile % 6) * 8 + (in & 7);
    y = by * 48 + (tile / 6) * 8 + (in >> 3);
    return x < F.W && y < F.H;
}

// What screen_ray reads of the camera record, with its two differences formed as it forms them.
struct CamTileView { double o[3], tl[3], ex[3], ey[3], w, h; };
template <class CAM>
FRAY_CERT_FN CamTileView cam_tile_view(const CAM& C)
{
    CamTileView V;
    for (int k = 0; k < 3; k++) { V.o[k] = C.pos[k]; V.tl[k] = C.topLeft[k]; V.ex[k] = C.topRight[k] - C.topLeft[k]; V.ey[k] = C.bottomLeft[k] - C.topLeft[k]; }
    V.w = C.w; V.h = C.h;
    return V;
}

// The four corner directions of the tile with the origin (x0, y0), Q and (R_t).
struct CamTileRays { double q[4][3]; double Q; bool range; };
FRAY_CERT_FN CamTileRays cam_tile_rays(const CamTileView& V, int x0, int y0)
{
    CamTileRays R;
    double S2 = 0;
    {
        double a = 0, b = 0, c = 0;
        for (int k = 0; k < 3; k++) {
            a = __builtin_fabs(V.tl[k]) > a ? __builtin_fabs(V.tl[k]) : a;
            b = __builtin_fabs(V.ex[k]) > b ? __builtin_fabs(V.ex[k]) : b;
            c = __builtin_fabs(V.ey[k]) > c ? __builtin_fabs(V.ey[k]) : c;
        }
        S2 = 2 * (a + b + c);
    }
    bool ok = V.w > 0 && V.h > 0 && (double)(x0 + 8) <= 2 * V.w && (double)(y0 + 8) <= 2 * V.h;
    double Q = 0;
    for (int c = 0; c < 4; c++) {
        const double x = (double)(x0 + ((c & 1) ? 8 : 0)), y = (double)(y0 + ((c & 2) ? 8 : 0));
        const double fx = x / V.w, fy = y / V.h;
        double s = 0;
        for (int k = 0; k < 3; k++) { R.q[c][k] = V.tl[k] + V.ex[k] * fx + V.ey[k] * fy; s += __builtin_fabs(R.q[c][k]); }      // (screen_ray's expression)
        ok = ok & (s >= 0x1p-40) & (s <= 0x1p40) & (64 * s >= S2);            // (false for a NaN or an infinity)
        Q = s > Q ? s : Q;
    }
    bool dominant = false;
    for (int k = 0; k < 3; k++) {
        double lo = R.q[0][k], hi = R.q[0][k];
        for (int c = 1; c < 4; c++) { lo = R.q[c][k] < lo ? R.q[c][k] : lo; hi = R.q[c][k] > hi ? R.q[c][k] : hi; }
        dominant = dominant | (lo >= 0x1p-8 * Q) | (hi <= -0x1p-8 * Q);
    }
    for (int k = 0; k < 3; k++) ok = ok & (__builtin_fabs(V.o[k]) < 1e9);      // (false for a NaN)
    R.Q = Q;
    R.range = ok & dominant;
    return R;
}

// (R_t) and (B_t) for one record (DCamSkip, DGateTight): every ray of the tile passes the record's box part.
template <class GT>
FRAY_CERT_FN bool tile_surely_misses_box(const GT& T, const CamTileView& V, const CamTileRays& R)
{
    if (!R.range) return false;
    const double sc = FRAY_CAMTILE_SCALE, Q = R.Q;
    double p[3], H[3], omax = 0, pmax = 0;
    for (int k = 0; k < 3; k++) {
        p[k] = V.o[k] - (double)T.cf[k];
        omax = __builtin_fabs(V.o[k]) > omax ? __builtin_fabs(V.o[k]) : omax;
        pmax = __builtin_fabs(p[k]) > pmax ? __builtin_fabs(p[k]) : pmax;
    }
    const double slack = sc * 0x1p-19 * (omax + pmax);
    const double eta = sc * 0x1p-21 * (omax + (double)T.Mf) + slack;
    for (int k = 0; k < 3; k++) H[k] = (double)T.hf[k] + eta;
    bool miss = false;
    for (int k = 0; k < 3; k++) {
        double lo = R.q[0][k], hi = R.q[0][k];
        for (int c = 1; c < 4; c++) { lo = R.q[c][k] < lo ? R.q[c][k] : lo; hi = R.q[c][k] > hi ? R.q[c][k] : hi; }
        miss = miss | ((p[k] > H[k]) & (lo >= 0)) | ((p[k] < -H[k]) & (hi <= 0));
    }
    const double g = 1 + sc * 0x1p-20, sl = slack * Q;
    for (int k = 0; k < 3; k++) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        double lo = 0, hi = 0, rmax = 0;
        for (int c = 0; c < 4; c++) {
            const double L = R.q[c][a] * p[b] - R.q[c][b] * p[a];
            const double r = __builtin_fabs(R.q[c][b]) * H[a] + __builtin_fabs(R.q[c][a]) * H[b];
            lo = (c == 0 || L < lo) ? L : lo; hi = (c == 0 || L > hi) ? L : hi;
            rmax = r > rmax ? r : rmax;
        }
        const double bound = rmax * g + sl + sc * 0x1p-40 * Q * (H[a] + H[b]);
        miss = miss | (lo > bound) | (hi < -bound);
    }
    return miss;
}
// (G_t) for one record: every ray of the tile passes the record's guard.
template <class GT>
FRAY_CERT_FN bool tile_surely_guarded(const GT& T, const CamTileRays& R)
{
    bool guard = true;
    if (FRAY_CAMTILE_SCALE) {
        const double gd = (double)T.guard * (1 + 0x1p-20) * R.Q;
        for (int j = 0; j < T.nDirs; j++) {
            double lo = 0, hi = 0;
            for (int c = 0; c < 4; c++) {
                const double f = (double)T.nf[j][0] * R.q[c][0] + (double)T.nf[j][1] * R.q[c][1] + (double)T.nf[j][2] * R.q[c][2];
                lo = (c == 0 || f < lo) ? f : lo; hi = (c == 0 || f > hi) ? f : hi;
            }
            guard = guard & ((lo > gd) | (hi < -gd));
        }
    }
    return guard;
}
// The whole tile certificate for one record.
template <class GT>
FRAY_CERT_FN bool tile_surely_misses_mesh(const GT& T, const CamTileView& V, const CamTileRays& R)
{
    return tile_surely_misses_box(T, V, R) & tile_surely_guarded(T, R);
}
