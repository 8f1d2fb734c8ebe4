// fr_cost_terms.hpp — the FrankaRidgeback objectives evaluated on one step record (kernels.hpp
// FR_REC stored layout, FR_NREC derived layout).  Shared by fr_step_cost_kernel (fr_cost.hip) and the rollout kernel's consumer
// waves (fr_coop.hip).
//
// AssistedManipulation::get_cost (assisted_manipulation.cpp:58-128) and TrackPoint::get_cost
// (frankaridgeback/objective/track_point.cpp:10-34), term order kept.  The joint-limit and
// velocity sums keep the association of the lane sums they replaced: (joints 0..5) + (6..11).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "device_common.hpp"
#include "engine_types.hpp"
#include "kernels.hpp"
#include "fsincos.hpp"

namespace mppi_cost {

using namespace mppi_eng;
using mppi_dev::smin;

constexpr int CK_ASSISTED_MANIPULATION = 1, CK_TRACK_POINT = 3;   // mppi_cost_kind

// x / d from v_rcp_f64 and one Newton correction applied to the product (four ops; the rcp's
// 2.8e-8 relative error squares to ~1e-15, against the IEEE quotient's ten-op sequence).  Only
// for barrier quotients, whose distance d from the bound is kept at or above 2^-512.  Below about
// 2^-1022 the rcp is inf and the product overflows, and the result was NaN (inf * 0, inf - inf)
// where the barrier is 0 (x = 0: the fingers' scale-0 barriers) or its maximum cost; a bound of
// exactly 0.0 and a joint one subnormal inside it get there.  The barriers' values do not change
// for d >= 2^-512, and below it x / 2^-512 is what x / d is: 0 for x = 0, beyond any maximum cost
// for x > 0.  d <= 0 and a NaN d become 2^-512 too: there the barriers select `over`.
__device__ __forceinline__ double fquot(double x, double d)
{
    d = __builtin_fmax(d, 0x1p-512);
    const double r = __builtin_amdgcn_rcp(d);
    const double t = x * r;
    const double e = __builtin_fma(-d, r, 1.0);
    return __builtin_fma(t, e, t);
}

// AssistedManipulation barriers (assisted_manipulation.cpp), written as selects: `under` strictly
// inside the bound, `over` on it, beyond it and for a NaN v (whose `over` is NaN, as the
// reference's min(scale / NaN, max) is)
__device__ __forceinline__ double right_barrier(double bound, double scale, double mx, double v)
{
    const double d = v - bound;
    const double over = mx + scale * (d * d);
    const double under = smin(fquot(scale, bound - v), mx);
    return (v < bound) ? under : over;
}
__device__ __forceinline__ double left_barrier(double bound, double scale, double mx, double v)
{
    const double d = bound - v;
    const double over = mx + scale * (d * d);
    const double under = smin(fquot(scale, v - bound), mx);
    return (v > bound) ? under : over;
}
__device__ __forceinline__ double right_barrier(const DevBarrier &b, double v) { return right_barrier(b.bound, b.scale, b.max, v); }
__device__ __forceinline__ double left_barrier(const DevBarrier &b, double v) { return left_barrier(b.bound, b.scale, b.max, v); }

// ---- the kinematic link-position model (mppi_set_link_positions) -------------------------------
// get_link_position(L) = the world translation of body L - 1 at the last calculate().  A step
// record holds x_k and the kinematics of the calculate() before it, which ran at q_{k-1} (at q_0
// for record 0: set_state's).  The rollout's Euler step is q_k = q_{k-1} + qd_k dt for every joint
// (the base's too: its qd is overwritten before the step), so the record itself gives that
// configuration back, q_{k-1} = q_k - qd_k dt to one rounding of q: no record is widened and no
// lane reads the previous step's record (which another workgroup may have written, the relay).
// first: record 0.
__device__ __forceinline__ double lagged_q(double q, double qd, double dt, bool first)
{
    return first ? q : __builtin_fma(-qd, dt, q);
}

// World translations of bodies 2..9 (the sphere links PIVOT, PANDA_LINK1..7) at joint positions
// qj[0..9]: fk_bodies' chain (fr_object.hip), pose_i = pose_parent o placement_i o joint_i, term for
// term, with the rollout kernel's fsincos.  Bodies 0..9 are one chain (FR_PARENT[i] = i - 1).
// R9 (or null): body 9's world rotation, row-major, which the chain carries to its end anyway
__device__ __forceinline__ void link_fk(const DevModel &M, const double *qj, double (*lp)[3], double *R9 = nullptr)
{
    const SinCosK K = sincos_constants();
    double R[9], p[3];
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const DevBody &b = M.b[i];
        double Rl[9], pl[3];
        if (FR_KIND[i] == KIND_RZ) {
            double s, c;
            fsincos(qj[i], &s, &c, K);
#pragma unroll
            for (int r = 0; r < 3; r++) {
                Rl[3 * r + 0] = b.R[3 * r + 0] * c + b.R[3 * r + 1] * s;
                Rl[3 * r + 1] = b.R[3 * r + 0] * (-s) + b.R[3 * r + 1] * c;
                Rl[3 * r + 2] = b.R[3 * r + 2];
                pl[r] = b.p[r];
            }
        } else {
            const int col = FR_KIND[i] == KIND_PX ? 0 : 1;
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int k = 0; k < 3; k++) Rl[3 * r + k] = b.R[3 * r + k];
                pl[r] = b.p[r] + b.R[3 * r + col] * qj[i];
            }
        }
        if (i == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = Rl[k];
#pragma unroll
            for (int k = 0; k < 3; k++) p[k] = pl[k];
        } else {
            double Rn[9], pn[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int cc = 0; cc < 3; cc++) Rn[3 * r + cc] = (R[3 * r] * Rl[cc] + R[3 * r + 1] * Rl[3 + cc]) + R[3 * r + 2] * Rl[6 + cc];
                pn[r] = p[r] + ((R[3 * r] * pl[0] + R[3 * r + 1] * pl[1]) + R[3 * r + 2] * pl[2]);
            }
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = Rn[k];
#pragma unroll
            for (int k = 0; k < 3; k++) p[k] = pn[k];
        }
        if (i >= SC_LINK0 - 1) {
#pragma unroll
            for (int k = 0; k < 3; k++) lp[i - (SC_LINK0 - 1)][k] = p[k];
        }
    }
    if (R9) {
#pragma unroll
        for (int k = 0; k < 9; k++) R9[k] = R[k];
    }
}

// self_collision_cost over the 20 sphere pairs, in the reference's pair order, on the sphere links'
// positions lp[link - 3]: AssistedManipulation passes distance - radii through the left barrier
// (assisted_manipulation.cpp:127-153), TrackPoint radii - distance (track_point.cpp:118-144).
template <bool TP>
__device__ __forceinline__ double self_collision_term(const DevCost &Cs, const double (*lp)[3])
{
    constexpr int A[SC_PAIRS] = {0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5};
    constexpr int B[SC_PAIRS] = {3, 4, 5, 6, 7, 3, 4, 5, 6, 7, 4, 5, 6, 7, 5, 6, 7, 6, 7, 7};
    double cost = 0.0;
#pragma unroll
    for (int n = 0; n < SC_PAIRS; n++) {
        const double d0 = lp[A[n]][0] - lp[B[n]][0], d1 = lp[A[n]][1] - lp[B[n]][1], d2 = lp[A[n]][2] - lp[B[n]][2];
        const double distance = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        const double radii = Cs.sc_radii[A[n]] + Cs.sc_radii[B[n]];
        cost += left_barrier(Cs.sc_limit, TP ? radii - distance : distance - radii);
    }
    return cost;
}

// The term of one step record from its own (q, qd) pairs at pq[2j], pq[2j + 1]
template <bool TP>
__device__ __forceinline__ double record_self_collision(const DevCost &Cs, const DevModel &M, const double *pq, double dt, bool first)
{
    double qj[10], lp[SC_LINKS][3];
#pragma unroll
    for (int j = 0; j < 10; j++) qj[j] = lagged_q(pq[2 * j], pq[2 * j + 1], dt, first);
    link_fk(M, qj, lp);
    return self_collision_term<TP>(Cs, lp);
}

// What the kinematic mode's objective needs beside the record: the model and the rollout's time step
struct LinkModel {
    const DevModel *model;
    double dt;
};

// ---- environment obstacles (mppi_set_obstacle_avoidance, mppi_set_obstacles) --------------------
// The step's obstacle term: sum over the table's obstacles o, in order, and over the robot's points
// i of mask_o, in order, of Left(limit)(clearance).  The points are the eight sphere links lp[0..7]
// (link_fk: lagged like the self-collision term's) and the record's grasp-frame position ee; obstacle
// o sits at position + velocity tau_k, tau_k = (t0 + k dt) - t_ref.  A sphere's clearance is
// |p - c| - (radii[i] + radius); a half-space's n . (p - c) - radii[i], no square root.  k and the
// points are the lane's; the table and o are the wave's: a runtime loop over count, and through an
// ObstacleTableK pointer (the rollouts) every table read is a scalar load.  The products and sums
// of tau_k and c are rounded one by one, as the host reference writes them.
// TP: const ObstacleTable * (the device object: its table is a kernel argument) or ObstacleTableK.
template <typename TP>
__device__ __forceinline__ double obstacle_term(TP T, const double (*lp)[3], const double *ee, double dt, int k)
{
    const double tau = __dsub_rn(__dadd_rn(T->t0, __dmul_rn((double)k, dt)), T->t_ref);
    const int count = T->count;
    const int n = count < OB_MAX ? count : OB_MAX;   // (never past the table, whatever it holds)
    const double bound = T->limit.bound, scale = T->limit.scale, mx = T->limit.max;
    double term = 0.0;
#pragma unroll 1
    for (int o = 0; o < n; o++) {
        const double c0 = __dadd_rn(T->ob[o].position[0], __dmul_rn(T->ob[o].velocity[0], tau));
        const double c1 = __dadd_rn(T->ob[o].position[1], __dmul_rn(T->ob[o].velocity[1], tau));
        const double c2 = __dadd_rn(T->ob[o].position[2], __dmul_rn(T->ob[o].velocity[2], tau));
        const unsigned mask = T->ob[o].mask;
        if (T->ob[o].kind == OB_HALF_SPACE) {
            const double n0 = T->ob[o].normal[0], n1 = T->ob[o].normal[1], n2 = T->ob[o].normal[2];
#pragma unroll
            for (int i = 0; i < OB_POINTS; i++) {
                const double *p = i < SC_LINKS ? lp[i] : ee;
                const double v = ((n0 * (p[0] - c0) + n1 * (p[1] - c1)) + n2 * (p[2] - c2)) - T->radii[i];
                const double b = left_barrier(bound, scale, mx, v);
                term += ((mask >> i) & 1u) ? b : 0.0;
            }
        } else {
            const double ro = T->ob[o].radius;
#pragma unroll
            for (int i = 0; i < OB_POINTS; i++) {
                const double *p = i < SC_LINKS ? lp[i] : ee;
                const double d0 = p[0] - c0, d1 = p[1] - c1, d2 = p[2] - c2;
                const double v = sqrt((d0 * d0 + d1 * d1) + d2 * d2) - (T->radii[i] + ro);
                const double b = left_barrier(bound, scale, mx, v);
                term += ((mask >> i) & 1u) ? b : 0.0;
            }
        }
    }
    return term;
}

// ---- capsules (mppi_set_obstacle_capsules): the links between the points, and capsule obstacles ----
// Robot segment s joins points s and s + 1 (the pairs are compile-time indices: the link coordinates
// stay in registers) with radius seg_radii[s], selected by mask bit 16 + s; an OB_CAPSULE obstacle is
// the segment c -> c + normal with its radius (include/mppi_amd.h has the definition).  Everything that
// decides a guard - A, E, B, den, t - is rounded operation by operation, as the host reference writes it.
__device__ __forceinline__ double dot3_rn(double a0, double a1, double a2, double b0, double b1, double b2)
{
    return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}
__device__ __forceinline__ double clamp01(double x)
{
    x = (x < 0.0) ? 0.0 : x;
    return (x > 1.0) ? 1.0 : x;
}

// The distance between segment a -> b and segment c -> c + e, E = e . e: Ericson's closest-point form
// with exact-zero guards only.  One straight line of selects: the clamps and the two re-solves of s
// differ per lane.  With E = 0 the quotient by E is NaN or inf and is selected away (t = 0 and the
// t < 0 re-solve, s = clamp(-C / A)); with A = 0, d1 = 0 makes B = C = den = 0, so s0 = 0 and t is
// clamp(F / E), and the re-solved s (0 / 0) is selected away.
__device__ __forceinline__ double segment_distance(const double *a, const double *b, double c0, double c1, double c2, double e0,
                                                   double e1, double e2, double E)
{
    const double x0 = __dsub_rn(b[0], a[0]), x1 = __dsub_rn(b[1], a[1]), x2 = __dsub_rn(b[2], a[2]);
    const double r0 = __dsub_rn(a[0], c0), r1 = __dsub_rn(a[1], c1), r2 = __dsub_rn(a[2], c2);
    const double A = dot3_rn(x0, x1, x2, x0, x1, x2), F = dot3_rn(e0, e1, e2, r0, r1, r2);
    const double Cc = dot3_rn(x0, x1, x2, r0, r1, r2), B = dot3_rn(x0, x1, x2, e0, e1, e2);
    const double den = __dsub_rn(__dmul_rn(A, E), __dmul_rn(B, B));
    const double sq = clamp01(__ddiv_rn(__dsub_rn(__dmul_rn(B, F), __dmul_rn(Cc, E)), den));
    const double s0 = (den > 0.0) ? sq : 0.0;
    const double tg = __ddiv_rn(__dadd_rn(__dmul_rn(B, s0), F), E);
    const bool ez = E == 0.0, lo = ez || tg < 0.0, hi = !lo && tg > 1.0;
    const double sr = clamp01(__ddiv_rn(lo ? -Cc : __dsub_rn(B, Cc), A));
    double s = (lo || hi) ? sr : s0;
    s = (A == 0.0) ? 0.0 : s;
    const double t = lo ? 0.0 : (hi ? 1.0 : tg);
    const double d0 = __dsub_rn(__dadd_rn(a[0], __dmul_rn(s, x0)), __dadd_rn(c0, __dmul_rn(t, e0)));
    const double d1 = __dsub_rn(__dadd_rn(a[1], __dmul_rn(s, x1)), __dadd_rn(c1, __dmul_rn(t, e1)));
    const double d2 = __dsub_rn(__dadd_rn(a[2], __dmul_rn(s, x2)), __dadd_rn(c2, __dmul_rn(t, e2)));
    return sqrt(dot3_rn(d0, d1, d2, d0, d1, d2));
}

// The end points of robot segment s (wave-uniform), each case by name: the link coordinates stay in
// registers, and one copy of the distance serves the eight segments
__device__ __forceinline__ void segment_ends(const double (*lp)[3], const double *ee, int s, double *a, double *b)
{
#define SEG_CASE(n, P, Q) case n: for (int i = 0; i < 3; i++) { a[i] = (P)[i]; b[i] = (Q)[i]; } break;
    switch (s) {
        SEG_CASE(0, lp[0], lp[1]) SEG_CASE(1, lp[1], lp[2]) SEG_CASE(2, lp[2], lp[3]) SEG_CASE(3, lp[3], lp[4])
        SEG_CASE(4, lp[4], lp[5]) SEG_CASE(5, lp[5], lp[6]) SEG_CASE(6, lp[6], lp[7])
        default: for (int i = 0; i < 3; i++) { a[i] = lp[7][i]; b[i] = ee[i]; } break;
    }
#undef SEG_CASE
}

// The step's term with capsules: per obstacle, in order, the masked points in order (bits 0..8), then
// the masked segments in order (bits 16..23), each clearance through Left(limit).  The kind and the
// masks are the wave's: the kind branch and each segment's mask test are scalar branches (a segment
// that no obstacle selects costs nothing), the table reads scalar loads.  A sphere is the capsule
// with e = 0; its points' clearances are obstacle_term's, expression for expression (q = c exactly).
// The eight segments are a rolled loop over one copy of the distance (unrolled, the x kernel, which holds
// the objective twice, was 16 KB larger and four variants spilled where their obstacle twins did not);
// segment_ends picks the end points by name.
template <typename TP>
__device__ __forceinline__ double capsule_term(TP T, const double (*lp)[3], const double *ee, double dt, int k)
{
    const double tau = __dsub_rn(__dadd_rn(T->t0, __dmul_rn((double)k, dt)), T->t_ref);
    const int count = T->count;
    const int n = count < OB_MAX ? count : OB_MAX;   // (never past the table, whatever it holds)
    const double bound = T->limit.bound, scale = T->limit.scale, mx = T->limit.max;
    double term = 0.0;
#pragma unroll 1
    for (int o = 0; o < n; o++) {
        const double c0 = __dadd_rn(T->ob[o].position[0], __dmul_rn(T->ob[o].velocity[0], tau));
        const double c1 = __dadd_rn(T->ob[o].position[1], __dmul_rn(T->ob[o].velocity[1], tau));
        const double c2 = __dadd_rn(T->ob[o].position[2], __dmul_rn(T->ob[o].velocity[2], tau));
        const unsigned mask = T->ob[o].mask;
        const int kind = T->ob[o].kind;
        if (kind == OB_HALF_SPACE) {
            const double n0 = T->ob[o].normal[0], n1 = T->ob[o].normal[1], n2 = T->ob[o].normal[2];
#pragma unroll
            for (int i = 0; i < OB_POINTS; i++) {
                const double *p = i < SC_LINKS ? lp[i] : ee;
                const double v = ((n0 * (p[0] - c0) + n1 * (p[1] - c1)) + n2 * (p[2] - c2)) - T->radii[i];
                const double b = left_barrier(bound, scale, mx, v);
                term += ((mask >> i) & 1u) ? b : 0.0;
            }
#pragma unroll 1
            for (int s = 0; s < OB_SEGMENTS; s++) {
                if ((mask >> (OB_SEGMENT_BIT0 + s)) & 1u) {
                    double p[3], q[3];
                    segment_ends(lp, ee, s, p, q);
                    const double hp = (n0 * (p[0] - c0) + n1 * (p[1] - c1)) + n2 * (p[2] - c2);
                    const double hq = (n0 * (q[0] - c0) + n1 * (q[1] - c1)) + n2 * (q[2] - c2);
                    term += left_barrier(bound, scale, mx, ((hq < hp) ? hq : hp) - T->seg_radii[s]);
                }
            }
        } else {
            const bool cap = kind == OB_CAPSULE;
            const double e0 = cap ? T->ob[o].normal[0] : 0.0, e1 = cap ? T->ob[o].normal[1] : 0.0, e2 = cap ? T->ob[o].normal[2] : 0.0;
            const double E = dot3_rn(e0, e1, e2, e0, e1, e2);
            const double ro = T->ob[o].radius;
#pragma unroll
            for (int i = 0; i < OB_POINTS; i++) {
                const double *p = i < SC_LINKS ? lp[i] : ee;
                // the point is the segment (p, p): s = 0, t = clamp(F / E), 0 with E = 0
                const double F = dot3_rn(e0, e1, e2, __dsub_rn(p[0], c0), __dsub_rn(p[1], c1), __dsub_rn(p[2], c2));
                const double t = (E == 0.0) ? 0.0 : clamp01(__ddiv_rn(F, E));
                const double d0 = p[0] - __dadd_rn(c0, __dmul_rn(t, e0)), d1 = p[1] - __dadd_rn(c1, __dmul_rn(t, e1));
                const double d2 = p[2] - __dadd_rn(c2, __dmul_rn(t, e2));
                const double v = sqrt((d0 * d0 + d1 * d1) + d2 * d2) - (T->radii[i] + ro);
                const double b = left_barrier(bound, scale, mx, v);
                term += ((mask >> i) & 1u) ? b : 0.0;
            }
#pragma unroll 1
            for (int s = 0; s < OB_SEGMENTS; s++) {
                if ((mask >> (OB_SEGMENT_BIT0 + s)) & 1u) {
                    double a[3], b[3];
                    segment_ends(lp, ee, s, a, b);
                    const double d = segment_distance(a, b, c0, c1, c2, e0, e1, e2, E);
                    term += left_barrier(bound, scale, mx, d - (T->seg_radii[s] + ro));
                }
            }
        }
    }
    return term;
}

// ---- the distance field (mppi_set_distance_field_avoidance, mppi_set_distance_field) -------------
// The sensed environment as a signed-distance grid (include/mppi_amd.h has the definition): the
// step's term is the sum of Left(limit)(D(p) - radius) over the masked points in order, then over
// the masked segments in order, each at its `samples` interior points a + phi_j (b - a).  D is the
// trilinear interpolant of the cell that holds p, z then y then x, every operation rounded by itself.
//
// field_cell: the cell and the fractions of one world point.  The cell index is clamped twice, as a
// double before the conversion (fmax and fmin take a NaN to the bound, so the conversion is always in
// range) and as an integer after it, on every lane whatever it holds: the address below never comes
// from an unclamped index, and with dims >= 2 (the host's check) all eight corners lie in the grid.
// st: 0 inside, 1 outside (contributes 0), 2 a NaN coordinate (NaN).
typedef const __attribute__((address_space(1))) float *FieldGrid;
struct FieldCell {
    int idx, st;
    double f[3];
};
template <typename TP>
__device__ __forceinline__ FieldCell field_cell(TP T, const double *p)
{
    // plain operators under contract(off): __dmul_rn and __dadd_rn are inline functions of plain operators
    // that carry the translation unit's contraction, and once inlined their product and sum fuse into an FMA
#pragma clang fp contract(off)
    FieldCell c;
    int i[3];
    bool inside = true, nan = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int n = T->field.dims[a];
        const double g = (p[a] - T->field.origin[a]) * T->field.inv_voxel;
        inside = inside && g >= 0.0 && g <= (double)(n - 1);
        nan = nan || g != g;
        int ia = (int)fmin(fmax(g, 0.0), (double)(n - 2));
        asm("" : "+v"(ia));   // (the integer clamp stays: the compiler may not reason it away from the double's range)
        ia = ia > n - 2 ? n - 2 : ia;
        ia = ia < 0 ? 0 : ia;
        i[a] = ia;
        c.f[a] = g - (double)ia;
    }
    c.idx = (i[0] * T->field.dims[1] + i[1]) * T->field.dims[2] + i[2];
    c.st = nan ? 2 : (inside ? 0 : 1);
    return c;
}
__device__ __forceinline__ double field_lerp(double a, double b, double f)
{
#pragma clang fp contract(off)
    return a + f * (b - a);
}

// The sampled unit u (wave-uniform): 0..8 the points (the segment (p, p)), 9..16 the segments, each
// case by name like segment_ends, so that the link coordinates stay in registers
__device__ __forceinline__ void field_ends(const double (*lp)[3], const double *ee, int u, double *a, double *b)
{
#define FLD_CASE(n, P, Q) case n: for (int i = 0; i < 3; i++) { a[i] = (P)[i]; b[i] = (Q)[i]; } break;
    switch (u) {
        FLD_CASE(0, lp[0], lp[0]) FLD_CASE(1, lp[1], lp[1]) FLD_CASE(2, lp[2], lp[2]) FLD_CASE(3, lp[3], lp[3])
        FLD_CASE(4, lp[4], lp[4]) FLD_CASE(5, lp[5], lp[5]) FLD_CASE(6, lp[6], lp[6]) FLD_CASE(7, lp[7], lp[7])
        FLD_CASE(8, ee, ee)
        FLD_CASE(9, lp[0], lp[1]) FLD_CASE(10, lp[1], lp[2]) FLD_CASE(11, lp[2], lp[3]) FLD_CASE(12, lp[3], lp[4])
        FLD_CASE(13, lp[4], lp[5]) FLD_CASE(14, lp[5], lp[6]) FLD_CASE(15, lp[6], lp[7])
        default: for (int i = 0; i < 3; i++) { a[i] = lp[7][i]; b[i] = ee[i]; } break;
    }
#undef FLD_CASE
}

// The step's field term.  One rolled loop over the samples around one copy of the sample, in two
// halves a sample apart: a trip finds the next sample's cell and issues its eight corner loads (the
// only per-lane memory reads; everything else is the table's, scalar loads), then interpolates the
// sample before it and runs its barrier while those loads are in flight.  The loop's control - the
// masks, the unit and the sample within it - is the wave's; a point is sampled as it is, a segment at
// a + phi (b - a).  No field (a null grid): nothing is read.
template <typename TP>
__device__ __forceinline__ double field_term(TP T, const double (*lp)[3], const double *ee)
{
#pragma clang fp contract(off)
    if (T->field.grid == nullptr) return 0.0;
    // (global memory, known as such: global_load, not flat_load; the base is the wave's, from the table)
    const FieldGrid grid = (FieldGrid) reinterpret_cast<uint64_t>(T->field.grid);
    const int nz = T->field.dims[2], nyz = T->field.dims[1] * nz;
    const unsigned mask = T->field.mask;
    int m = T->field.samples;
    m = m < 0 ? 0 : (m > OB_FIELD_SAMPLES ? OB_FIELD_SAMPLES : m);   // (never past phi, whatever the table holds)
    // the units left: bits 0..8 the points, bits 9..16 the segments (none with no samples)
    unsigned rem = (mask & 0x1FFu) | (m > 0 ? ((mask >> OB_SEGMENT_BIT0) & 0xFFu) << OB_POINTS : 0u);
    const double bound = T->limit.bound, scale = T->limit.scale, mx = T->limit.max;
    double term = 0.0;
    int u = 0, j = 0, cnt = 0;
    bool cur = false;                      // a sample is in flight
    float c[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    double f[3] = {0.0, 0.0, 0.0}, rad = 0.0;
    int st = 1;
#pragma unroll 1
    for (;;) {
        bool have = true;
        if (j + 1 < cnt) j++;
        else if (rem) {
            u = __builtin_ctz(rem);
            rem &= rem - 1u;
            j = 0;
            cnt = u >= OB_POINTS ? m : 1;
        } else have = false;
        float nc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        FieldCell cell{0, 1, {0.0, 0.0, 0.0}};
        double nrad = 0.0;
        if (have) {
            double a[3], b[3], p[3];
            field_ends(lp, ee, u, a, b);
            const bool seg = u >= OB_POINTS;
            const double phi = seg ? T->field.phi[j] : 0.0;
            nrad = seg ? T->seg_radii[u - OB_POINTS] : T->radii[seg ? 0 : u];
#pragma unroll
            for (int i = 0; i < 3; i++) p[i] = seg ? a[i] + phi * (b[i] - a[i]) : a[i];   // (a point is itself, also an infinite one: outside, 0)
            cell = field_cell(T, p);
            // eight dword loads: the z pair's upper address goes through an empty asm, so that the pair is
            // not merged into one 8-byte load at 4-byte alignment
            const FieldGrid g = grid + cell.idx;
            FieldGrid g1 = g + 1;
            asm("" : "+v"(g1));
            nc[0] = g[0];
            nc[1] = g1[0];
            nc[2] = g[nz];
            nc[3] = g1[nz];
            nc[4] = g[nyz];
            nc[5] = g1[nyz];
            nc[6] = g[nyz + nz];
            nc[7] = g1[nyz + nz];
        }
        if (cur) {
            const double z00 = field_lerp((double)c[0], (double)c[1], f[2]), z01 = field_lerp((double)c[2], (double)c[3], f[2]);
            const double z10 = field_lerp((double)c[4], (double)c[5], f[2]), z11 = field_lerp((double)c[6], (double)c[7], f[2]);
            const double y0 = field_lerp(z00, z01, f[1]), y1 = field_lerp(z10, z11, f[1]);
            const double D = field_lerp(y0, y1, f[0]);
            const double bv = left_barrier(bound, scale, mx, D - rad);
            term += st == 0 ? bv : (st == 1 ? 0.0 : __builtin_nan(""));
        }
        if (!have) break;
#pragma unroll
        for (int i = 0; i < 8; i++) c[i] = nc[i];
#pragma unroll
        for (int i = 0; i < 3; i++) f[i] = cell.f[i];
        rad = nrad;
        st = cell.st;
        cur = true;
    }
    return term;
}

__device__ __forceinline__ void grasp_rotation(const double *R9, const double *eeR, double *Ree);

// ---- the held object (mppi_set_held_object_avoidance, mppi_set_held_object) -----------------------
// Up to four spheres fixed in the grasp frame and the segments between consecutive ones
// (include/mppi_amd.h has the definition).  Held point i sits at h_i = p_ee + Ree c_i, p_ee the
// grasp-frame position that obstacle point 8 reads and Ree = R9 ee_R at the same lagged configuration
// (grasp_rotation); every operation of the sum is rounded by itself.  The four points are formed once
// per step; the table's reads - the object, the masks, the radii - are the wave's.
// HP: a pointer to the DevHeld (the table's, in the table's address space, or a kernel argument's)
template <typename HP>
__device__ __forceinline__ void held_points(HP Hd, const double *pe, const double *Ree, double (*h)[3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < OB_HELD_POINTS; i++) {
        const double cx = Hd->centres[i][0], cy = Hd->centres[i][1], cz = Hd->centres[i][2];
#pragma unroll
        for (int r = 0; r < 3; r++) h[i][r] = pe[r] + ((Ree[3 * r] * cx + Ree[3 * r + 1] * cy) + Ree[3 * r + 2] * cz);
    }
}

// The tested unit u (wave-uniform): 0..3 the held points (the segment (h, h)), 4..6 the held segments,
// each case by name so that the points stay in registers
__device__ __forceinline__ void held_ends(const double (*h)[3], int u, double *a, double *b)
{
#define HELD_CASE(n, P, Q) case n: for (int i = 0; i < 3; i++) { a[i] = (P)[i]; b[i] = (Q)[i]; } break;
    switch (u) {
        HELD_CASE(0, h[0], h[0]) HELD_CASE(1, h[1], h[1]) HELD_CASE(2, h[2], h[2]) HELD_CASE(3, h[3], h[3])
        HELD_CASE(4, h[0], h[1]) HELD_CASE(5, h[1], h[2])
        default: for (int i = 0; i < 3; i++) { a[i] = h[2][i]; b[i] = h[3][i]; } break;
    }
#undef HELD_CASE
}

// The held points and segments against the table's obstacles: capsule_term's clearances, expression for
// expression, with the held radii in place of the robot's.  Per obstacle, in order, the masked held
// points in order (bits 9..12), then the masked held segments in order (bits 24..26); a bit that names a
// point or segment the object does not have selects nothing.  Every mask test is a scalar branch.
template <typename TP>
__device__ __forceinline__ double held_obstacle_term(TP T, const double (*h)[3], int hc, double dt, int k)
{
    const double tau = __dsub_rn(__dadd_rn(T->t0, __dmul_rn((double)k, dt)), T->t_ref);
    const int count = T->count;
    const int n = count < OB_MAX ? count : OB_MAX;   // (never past the table, whatever it holds)
    const double bound = T->limit.bound, scale = T->limit.scale, mx = T->limit.max;
    const unsigned pm = (1u << hc) - 1u, sm = (1u << (hc - 1)) - 1u;
    double term = 0.0;
#pragma unroll 1
    for (int o = 0; o < n; o++) {
        const unsigned mask = T->ob[o].mask;
        const unsigned pb = (mask >> OB_HELD_POINT_BIT0) & pm, sb = (mask >> OB_HELD_SEGMENT_BIT0) & sm;
        if ((pb | sb) == 0u) continue;
        const double c0 = __dadd_rn(T->ob[o].position[0], __dmul_rn(T->ob[o].velocity[0], tau));
        const double c1 = __dadd_rn(T->ob[o].position[1], __dmul_rn(T->ob[o].velocity[1], tau));
        const double c2 = __dadd_rn(T->ob[o].position[2], __dmul_rn(T->ob[o].velocity[2], tau));
        const int kind = T->ob[o].kind;
        if (kind == OB_HALF_SPACE) {
            const double n0 = T->ob[o].normal[0], n1 = T->ob[o].normal[1], n2 = T->ob[o].normal[2];
#pragma unroll 1
            for (int i = 0; i < OB_HELD_POINTS; i++) {
                if ((pb >> i) & 1u) {
                    double p[3], q[3];
                    held_ends(h, i, p, q);
                    const double v = ((n0 * (p[0] - c0) + n1 * (p[1] - c1)) + n2 * (p[2] - c2)) - T->held.radii[i];
                    term += left_barrier(bound, scale, mx, v);
                }
            }
#pragma unroll 1
            for (int s = 0; s < OB_HELD_SEGMENTS; s++) {
                if ((sb >> s) & 1u) {
                    double p[3], q[3];
                    held_ends(h, OB_HELD_POINTS + s, p, q);
                    const double hp = (n0 * (p[0] - c0) + n1 * (p[1] - c1)) + n2 * (p[2] - c2);
                    const double hq = (n0 * (q[0] - c0) + n1 * (q[1] - c1)) + n2 * (q[2] - c2);
                    term += left_barrier(bound, scale, mx, ((hq < hp) ? hq : hp) - T->held.seg_radii[s]);
                }
            }
        } else {
            const bool cap = kind == OB_CAPSULE;
            const double e0 = cap ? T->ob[o].normal[0] : 0.0, e1 = cap ? T->ob[o].normal[1] : 0.0, e2 = cap ? T->ob[o].normal[2] : 0.0;
            const double E = dot3_rn(e0, e1, e2, e0, e1, e2);
            const double ro = T->ob[o].radius;
#pragma unroll 1
            for (int i = 0; i < OB_HELD_POINTS; i++) {
                if ((pb >> i) & 1u) {
                    double p[3], q[3];
                    held_ends(h, i, p, q);
                    // the point is the segment (p, p): s = 0, t = clamp(F / E), 0 with E = 0
                    const double F = dot3_rn(e0, e1, e2, __dsub_rn(p[0], c0), __dsub_rn(p[1], c1), __dsub_rn(p[2], c2));
                    const double t = (E == 0.0) ? 0.0 : clamp01(__ddiv_rn(F, E));
                    const double d0 = p[0] - __dadd_rn(c0, __dmul_rn(t, e0)), d1 = p[1] - __dadd_rn(c1, __dmul_rn(t, e1));
                    const double d2 = p[2] - __dadd_rn(c2, __dmul_rn(t, e2));
                    const double v = sqrt((d0 * d0 + d1 * d1) + d2 * d2) - (T->held.radii[i] + ro);
                    term += left_barrier(bound, scale, mx, v);
                }
            }
#pragma unroll 1
            for (int s = 0; s < OB_HELD_SEGMENTS; s++) {
                if ((sb >> s) & 1u) {
                    double a[3], b[3];
                    held_ends(h, OB_HELD_POINTS + s, a, b);
                    const double d = segment_distance(a, b, c0, c1, c2, e0, e1, e2, E);
                    term += left_barrier(bound, scale, mx, d - (T->held.seg_radii[s] + ro));
                }
            }
        }
    }
    return term;
}

// The held points and segments in the distance field: field_term's sample, operation for operation -
// the masked held points in order (the field's mask bits 9..12), then the masked held segments in order
// (bits 24..26), each at its `samples` interior points in order j.  One rolled loop around one copy of
// the sample; the corner loads are the only per-lane memory reads.  No field: nothing is read.
template <typename TP>
__device__ __forceinline__ double held_field_term(TP T, const double (*h)[3], int hc)
{
#pragma clang fp contract(off)
    if (T->field.grid == nullptr) return 0.0;
    const FieldGrid grid = (FieldGrid) reinterpret_cast<uint64_t>(T->field.grid);
    const int nz = T->field.dims[2], nyz = T->field.dims[1] * nz;
    const unsigned mask = T->field.mask;
    int m = T->field.samples;
    m = m < 0 ? 0 : (m > OB_FIELD_SAMPLES ? OB_FIELD_SAMPLES : m);   // (never past phi, whatever the table holds)
    const unsigned pm = (1u << hc) - 1u, sm = (1u << (hc - 1)) - 1u;
    // the units left: bits 0..3 the held points, bits 4..6 the held segments (none with no samples)
    unsigned rem = ((mask >> OB_HELD_POINT_BIT0) & pm) | (m > 0 ? ((mask >> OB_HELD_SEGMENT_BIT0) & sm) << OB_HELD_POINTS : 0u);
    const double bound = T->limit.bound, scale = T->limit.scale, mx = T->limit.max;
    double term = 0.0;
#pragma unroll 1
    while (rem) {
        const int u = __builtin_ctz(rem);
        rem &= rem - 1u;
        const bool seg = u >= OB_HELD_POINTS;
        const int cnt = seg ? m : 1;
        double a[3], b[3];
        held_ends(h, u, a, b);
        const double rad = seg ? T->held.seg_radii[u - OB_HELD_POINTS] : T->held.radii[seg ? 0 : u];
#pragma unroll 1
        for (int j = 0; j < cnt; j++) {
            const double phi = seg ? T->field.phi[j] : 0.0;
            double p[3];
#pragma unroll
            for (int i = 0; i < 3; i++) p[i] = seg ? a[i] + phi * (b[i] - a[i]) : a[i];   // (a point is itself)
            const FieldCell cell = field_cell(T, p);
            const FieldGrid g = grid + cell.idx;
            FieldGrid g1 = g + 1;
            asm("" : "+v"(g1));   // (eight dword loads, as field_term's)
            const float c0 = g[0], c1 = g1[0], c2 = g[nz], c3 = g1[nz], c4 = g[nyz], c5 = g1[nyz], c6 = g[nyz + nz], c7 = g1[nyz + nz];
            const double z00 = field_lerp((double)c0, (double)c1, cell.f[2]), z01 = field_lerp((double)c2, (double)c3, cell.f[2]);
            const double z10 = field_lerp((double)c4, (double)c5, cell.f[2]), z11 = field_lerp((double)c6, (double)c7, cell.f[2]);
            const double y0 = field_lerp(z00, z01, cell.f[1]), y1 = field_lerp(z10, z11, cell.f[1]);
            const double D = field_lerp(y0, y1, cell.f[0]);
            const double bv = left_barrier(bound, scale, mx, D - rad);
            term += cell.st == 0 ? bv : (cell.st == 1 ? 0.0 : __builtin_nan(""));
        }
    }
    return term;
}

// The step's held term: the obstacles' part, then the field's.  Nothing held: +0.0, and nothing but
// the object's count is read.
// h: the four world points, handed on to held_self_term (left alone where nothing is held)
template <typename TP>
__device__ __forceinline__ double held_term_at(TP T, const double *pe, const double *Ree, double dt, int k, double (*h)[3])
{
    int hc = T->held.count;
    hc = hc > OB_HELD_POINTS ? OB_HELD_POINTS : hc;   // (never past the object, whatever the table holds)
    if (hc <= 0) return 0.0;
    held_points(&T->held, pe, Ree, h);
    return held_obstacle_term(T, h, hc, dt, k) + held_field_term(T, h, hc);
}
template <typename TP>
__device__ __forceinline__ double held_term_at(TP T, const double *pe, const double *Ree, double dt, int k)
{
    double h[OB_HELD_POINTS][3];
    return held_term_at(T, pe, Ree, dt, k, h);
}

// ---- the held object against the robot's own segments (mppi_set_held_self_avoidance) ---------------
// The units the step tests (wave-uniform): bits 0..3 the masked held points, bits 4..6 the masked held
// segments, of those the current object has; 0 with no object, no configuration or no robot segment
// masked - then nothing but the counts and masks was read.
template <typename TP>
__device__ __forceinline__ unsigned held_self_units(TP T)
{
    int hc = T->held.count;
    hc = hc > OB_HELD_POINTS ? OB_HELD_POINTS : hc;
    if (hc <= 0) return 0u;
    if ((T->self.segments & OB_HELD_SELF_SEGMENTS) == 0u) return 0u;
    const unsigned pm = (1u << hc) - 1u, sm = (1u << (hc - 1)) - 1u;
    return T->self.units & (pm | (sm << OB_HELD_POINTS));
}

// The held units against the robot's segments (include/mppi_amd.h has the definition): capsule_term's
// segment clearance with the robot's segment a -> b first and the held unit c -> c + e second - a held
// point has e = 0, a held segment e = h_{s'+1} - h_s', one rounded subtraction a component - and
// v = d - (self.radii[s] + r_u).  Units in order u = 0..6, per unit the masked robot segments in order
// s = 0..7: two rolled loops around one copy of the distance; held_ends and segment_ends pick the ends by
// name.  rem: held_self_units, not 0; h: the step's held points, as held_term_at formed them.
template <typename TP>
__device__ __forceinline__ double held_self_term(TP T, unsigned rem, const double (*h)[3], const double (*lp)[3], const double *ee)
{
    const unsigned segs = T->self.segments & OB_HELD_SELF_SEGMENTS;
    const double bound = T->limit.bound, scale = T->limit.scale, mx = T->limit.max;
    double term = 0.0;
#pragma unroll 1
    while (rem) {
        const int u = __builtin_ctz(rem);
        rem &= rem - 1u;
        const bool seg = u >= OB_HELD_POINTS;
        double c[3], q[3];
        held_ends(h, u, c, q);
        const double e0 = seg ? __dsub_rn(q[0], c[0]) : 0.0, e1 = seg ? __dsub_rn(q[1], c[1]) : 0.0, e2 = seg ? __dsub_rn(q[2], c[2]) : 0.0;
        const double E = dot3_rn(e0, e1, e2, e0, e1, e2);
        const double ru = seg ? T->held.seg_radii[u - OB_HELD_POINTS] : T->held.radii[seg ? 0 : u];
        unsigned sl = segs;
#pragma unroll 1
        while (sl) {
            const int s = __builtin_ctz(sl);
            sl &= sl - 1u;
            double a[3], b[3];
            segment_ends(lp, ee, s, a, b);
            const double d = segment_distance(a, b, c[0], c[1], c[2], e0, e1, e2, E);
            term += left_barrier(bound, scale, mx, d - (T->self.radii[s] + ru));
        }
    }
    return term;
}

// The step's held term and, behind it, its held-self term (self): the points are formed once for both
template <typename TP>
__device__ __forceinline__ double held_terms(TP T, const double (*lp)[3], const double *pe, const double *R9, const double *eeR,
                                             double dt, int k, double &self)
{
    self = 0.0;
    if (T->held.count <= 0) return 0.0;
    double Ree[9], h[OB_HELD_POINTS][3];
    grasp_rotation(R9, eeR, Ree);
    const double held = held_term_at(T, pe, Ree, dt, k, h);
    const unsigned rem = held_self_units(T);
    if (rem) self = held_self_term(T, rem, h, lp, pe);
    return held;
}
// The held-self term alone at a grasp pose (Ree) and link positions: the read-out's and the device object's
template <typename TP>
__device__ __forceinline__ double held_self_term_at(TP T, const double (*lp)[3], const double *pe, const double *Ree)
{
    const unsigned rem = held_self_units(T);
    if (rem == 0u) return 0.0;
    double h[OB_HELD_POINTS][3];
    held_points(&T->held, pe, Ree, h);
    return held_self_term(T, rem, h, lp, pe);
}
// held_term_at from body 9's rotation where link_fk leaves it (R9) and the model's grasp placement
template <typename TP>
__device__ __forceinline__ double held_term(TP T, const double *pe, const double *R9, const double *eeR, double dt, int k)
{
    if (T->held.count <= 0) return 0.0;
    double Ree[9];
    grasp_rotation(R9, eeR, Ree);
    return held_term_at(T, pe, Ree, dt, k);
}

// An update's obstacle table as the rollouts' objective reads it: nothing writes it during a launch
// (obstacle_table_kernel ran before), so it is addressed in the constant address space, and its
// address is made the wave's by v_readfirstlane - it is the same on every lane, but where it hangs
// on the wave's row (the folded filter() row reads fsteps) the compiler cannot see that.  Uniform
// address and constant space together make every read of the table an s_load.
typedef const __attribute__((address_space(4))) ObstacleTable *ObstacleTableK;
__device__ __forceinline__ ObstacleTableK obstacle_table_of(const StepConst *steps, int H)
{
    const uint64_t a = reinterpret_cast<uint64_t>(steps + 2 * (int64_t)H);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return (ObstacleTableK)(((uint64_t)hi << 32) | lo);
}

// Where a lane's step finds its obstacles: the table behind its update's step constants and wrench
// rows (obstacle_table_of) and its step index k.  A wave of the x kernel's objective may hold rows
// of this update beside the folded filter() row, which reads the previous update's table: such a
// wave passes that table as ftab (else null) and frow on the row's lanes, and the term runs once
// per table, both times on scalar loads.
struct ObstacleRef {
    ObstacleTableK tab, ftab;
    bool frow;
    int k;
};
// TERM: OB_TERM_POINTS obstacle_term, OB_TERM_CAPSULES capsule_term, OB_TERM_FIELD capsule_term and then
// field_term, both from the same table - the folded filter() row's second pass so reads its own
// update's grid; OB_TERM_HELD (capsule_term + field_term) + held_term, the held object's from the same table
// too, with body 9's rotation R9 and the model's grasp placement eeR; OB_TERM_HELD_SELF that and then
// held_self_term on the same held points, ((capsule + field) + held) + self
template <int TERM = OB_TERM_POINTS>
__device__ __forceinline__ double obstacle_cost(const ObstacleRef &ob, const double (*lp)[3], const double *ee, double dt,
                                                const double *R9 = nullptr, const double *eeR = nullptr)
{
    double term = 0.0;
    const int np = ob.ftab ? 2 : 1;
#pragma unroll 1
    for (int pass = 0; pass < np; pass++) {
        const ObstacleTableK T = pass ? ob.ftab : ob.tab;
        double t;
        if constexpr (TERM == OB_TERM_HELD_SELF) {
            const double cf = capsule_term(T, lp, ee, dt, ob.k) + field_term(T, lp, ee);
            double self;
            const double held = held_terms(T, lp, ee, R9, eeR, dt, ob.k, self);
            t = (cf + held) + self;
        } else if constexpr (TERM == OB_TERM_HELD) t = (capsule_term(T, lp, ee, dt, ob.k) + field_term(T, lp, ee)) + held_term(T, ee, R9, eeR, dt, ob.k);
        else if constexpr (TERM == OB_TERM_FIELD) t = capsule_term(T, lp, ee, dt, ob.k) + field_term(T, lp, ee);
        else if constexpr (TERM == OB_TERM_CAPSULES) t = capsule_term(T, lp, ee, dt, ob.k);
        else t = obstacle_term(T, lp, ee, dt, ob.k);
        term = (pass == 0 || ob.frow) ? t : term;
    }
    return term;
}

// Per-joint parameters of the objective in LDS, joint j at Lj[j JS ..]: lower barrier (bound,
// scale, max), upper barrier, velocity weight - uniform loads next to their use instead of 84
// scalar registers the compiler loaded up front and spilled.  fr_cost.hip stages them with stride
// JT_STRIDE; the rollout kernel reads them from its body table.
constexpr int JT_STRIDE = 7;

// trajectory_cost's velocity part on the EE frame velocity (assisted_manipulation.cpp:237-290)
__device__ __forceinline__ double trajectory_term(const DevCost &Cs, const StepConst &sc, const double *vl)
{
    double proj = ((vl[0] * sc.target[0] + vl[1] * sc.target[1]) + vl[2] * sc.target[2]) / sc.tt;
    const double p0 = proj * sc.target[0], p1 = proj * sc.target[1], p2 = proj * sc.target[2];
    proj = copysign(1.0, proj) * sqrt((p0 * p0 + p1 * p1) + p2 * p2);
    const double err = fabs(sc.vtarget - proj);
    const double tc = sc.pos_cost + ((Cs.traj_vel_c + Cs.traj_vel_l * fabs(err)) + Cs.traj_vel_q * err * err);
    return sc.active ? tc : 0.0;
}

// manipulability_cost on J_a J_a^T (assisted_manipulation.cpp:224-235)
__device__ __forceinline__ double manipulability_term(const DevCost &Cs, const double *jj)
{
    const double m00 = jj[0], m01 = jj[1], m02 = jj[2], m11 = jj[3], m12 = jj[4], m22 = jj[5];
    const double det = (m00 * (m11 * m22 - m12 * m12) - m01 * (m01 * m22 - m12 * m02)) + m02 * (m01 * m12 - m11 * m02);
    double vol = sqrt(det);
    vol = isnan(vol) ? 1e-5 : ((vol < 1e-5) ? 1e-5 : ((1e5 < vol) ? 1e5 : vol));
    const double iv = 1.0 / vol;
    return (Cs.manip_c + Cs.manip_l * fabs(iv)) + Cs.manip_q * iv * iv;
}

// J v and J_a J_a^T of a stored record (kernels.hpp REC_S01 / REC_S2Q) by the chains the rollout
// kernel's lanes ran before r05, term for term: lane m of a row summed over the bodies i = 0..9, in
// order, acc = fma(x_i, y_i, acc) from acc = 0, with x_i = S_i[m] and y_i = qd_i for J v (m < 3),
// and x_i = S_i[a], y_i = S_i[b] (y_i = 0 for the base, i < 3) for the packed J_a J_a^T entry (a, b)
// - so the sums, and every cost, keep their bits.
__device__ __forceinline__ void kin_sums(const double2 *rec2, double *vl, double *jj)
{
    double s0[10], s1[10], s2[10], qd[10];
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const double2 a = rec2[REC_S01 / 2 + i], b = rec2[REC_S2Q / 2 + i];
        s0[i] = a.x;
        s1[i] = a.y;
        s2[i] = b.x;
        qd[i] = b.y;
    }
    const double *S[3] = {s0, s1, s2};
    constexpr int ja[6] = {0, 0, 0, 1, 1, 2}, jb[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int m = 0; m < 3; m++) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 10; i++) acc = __builtin_fma(S[m][i], qd[i], acc);
        vl[m] = acc;
    }
    // (the base's three terms of J_a J_a^T are fma(x, 0, +0) = +0 on the rows' chains, store_ks: a
    // chain that starts at body 3 from +0 has the same bits for finite S)
#pragma unroll
    for (int p = 0; p < 6; p++) {
        double acc = 0.0;
#pragma unroll
        for (int i = 3; i < 10; i++) acc = __builtin_fma(S[ja[p]][i], S[jb[p]][i], acc);
        jj[p] = acc;
    }
}

// The derived record (FR_NREC) of a stored one (FR_REC; a compact FR_REC_C record is one already)
__device__ __forceinline__ void derive_record(const double *rk, double *r, bool compact = false)
{
    const double2 *src = reinterpret_cast<const double2 *>(rk);
    const int n = compact ? FR_NREC / 2 : REC_VL / 2;
    for (int i = 0; i < n; i++) {
        const double2 v = src[i];
        r[2 * i] = v.x;
        r[2 * i + 1] = v.y;
    }
    if (!compact) kin_sums(src, r + REC_VL, r + REC_JJ);
    r[FR_NREC - 1] = 0.0;
}

// AssistedManipulation::get_cost at the record's state with its kinematics (KC: a compact record,
// J v and J_a J_a^T stored; else the 768-B record, whose motion subspaces they are formed from)
// LP: the kinematic link-position model - the self-collision term from the record's link positions
// (lm, first: record_self_collision) instead of the zero stub's constant
// OB (with LP): the obstacle term on the same link positions (ob: obstacle_cost), added after the
// reference's terms; the link FK then runs whether or not the self-collision switch is on.  OB_TERM_NONE,
// OB_TERM_POINTS (the nine points), OB_TERM_CAPSULES (points and segments, capsule obstacles) or
// OB_TERM_FIELD (the capsule term and the distance field's), or OB_TERM_HELD (those two and the held
// object's, which needs body 9's rotation from the same link FK), or OB_TERM_HELD_SELF (those three and
// the held object against the robot's segments)
template <bool EN, int JS, bool KC = false, int JG = 1, bool LP = false, int OB = OB_TERM_NONE>
__device__ __forceinline__ double assisted_manipulation_cost(const DevCost &Cs, const StepConst &sc, const double *r,
                                                             const double *Lj, const double2 *src, LinkModel lm = LinkModel{},
                                                             bool first = false, ObstacleRef ob = ObstacleRef{})
{
    static_assert(LP || !OB, "the obstacles read the kinematic link positions");
    double j0 = 0.0, j1 = 0.0, v0 = 0.0, v1 = 0.0;
    int off = 0;
    // JG joints at a time: their parameters are read after the previous group's terms (left to
    // itself the compiler hoisted all 84 LDS reads to the top: 168 registers live), and the group's
    // barrier chains interleave (one joint at a time, each v_rcp_f64 waited a wait state for its
    // reader: the trans forwarding hazard).  The sums add the joints in order either way.
#pragma unroll
    for (int j = 0; j < FR_NB; j += JG) {
        asm volatile("" : "+v"(off) : "v"(j < 6 ? j0 : j1));
        double lj[JG], lv[JG];
#pragma unroll
        for (int u = 0; u < JG; u++) {
            const double *P = Lj + off + u * JS;
            const double q = r[REC_QQD + 2 * (j + u)], vq = fabs(r[REC_QQD + 2 * (j + u) + 1]);
            lj[u] = left_barrier(P[0], P[1], P[2], q) + right_barrier(P[3], P[4], P[5], q);
            lv[u] = P[6] * (vq * vq);
        }
        off += JG * JS;
#pragma unroll
        for (int u = 0; u < JG; u++) {
            if (j + u < 6) { j0 += lj[u]; v0 += lv[u]; }
            else { j1 += lj[u]; v1 += lv[u]; }
        }
    }
    const double joint = j0 + j1, vel = v0 + v1;
    // the rest of the record (r holds the (q, qd) pairs only) is loaded through a pointer that
    // waits for the joint sums: the remaining terms start after them instead of interleaving with
    // them and holding their values live (two waves per SIMD instead of four)
    static_assert(REC_EE == 2 * FR_NB && REC_VL - REC_EE == 8, "record tail");
    // (the dependency rides on an index, not on the pointer: an opaque pointer loses its address
    // space, and its loads became flat_load, which wait for the LDS counter as well)
    double rest[REC_VL - REC_EE], yaw = r[REC_QQD + 4];
    int dep = 0;
    asm volatile("" : "+v"(dep), "+v"(yaw) : "v"(joint), "v"(vel));
    const double2 *tp = src + dep;
#pragma unroll
    for (int i = 0; i < (REC_VL - REC_EE) / 2; i++) {
        const double2 v = tp[REC_EE / 2 + i];
        rest[2 * i] = v.x;
        rest[2 * i + 1] = v.y;
    }
    double vl[3], jj[6];
    if constexpr (KC) {   // stored by the rows (REC_VL, REC_JJ)
        double kv[10];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const double2 v = tp[REC_VL / 2 + i];
            kv[2 * i] = v.x;
            kv[2 * i + 1] = v.y;
        }
#pragma unroll
        for (int i = 0; i < 3; i++) vl[i] = kv[i];
#pragma unroll
        for (int i = 0; i < 6; i++) jj[i] = kv[3 + i];
    } else {
        kin_sums(tp, vl, jj);   // from the stored record's motion subspaces
    }
    r = rest - REC_EE;   // r[REC_EE .. REC_VL) from here on
    double s, c;
    fsincos(yaw, &s, &c, sincos_constants());   // base yaw q_2
    const double *ee = r + REC_EE, *am = r + REC_AM;
    double wc = 0.0;
    {
        const double r22 = (1.0 - c) + c;
        const double fw0 = c, fw1 = s, fw2 = 0.0;
        const double off0 = (0.1 * c + (-s) * 0.0) + 0.0 * 0.15;
        const double off1 = (0.1 * s + c * 0.0) + 0.0 * 0.15;
        const double off2 = (0.0 * 0.1 + 0.0 * 0.0) + r22 * 0.15;
        const double rb2 = am[2] + off2;
        const double t0 = ee[0] - (am[0] + off0), t1 = ee[1] - (am[1] + off1), t2 = ee[2] - rb2;
        const double proj = ((t0 * fw0 + t1 * fw1) + t2 * fw2) / ((fw0 * fw0 + fw1 * fw1) + fw2 * fw2);
        wc += left_barrier(Cs.ws_infront, proj);
        wc += right_barrier(Cs.ws_reach, sqrt((t0 * t0 + t1 * t1) + t2 * t2));
        const double n1 = sqrt(t0 * t0 + t1 * t1);
        const double n2 = sqrt(fw0 * fw0 + fw1 * fw1);
        const double yaw = acos((t0 * fw0 + t1 * fw1) / n1 / n2);
        const double ay = fabs(yaw);
        const double yc = (Cs.yaw_c + Cs.yaw_l * fabs(ay)) + Cs.yaw_q * ay * ay;
        wc += isnan(yaw) ? 0.0 : yc;
        wc += left_barrier(Cs.ws_above, ee[2] - rb2);
    }
    if constexpr (OB) {
        // One link FK for the self-collision and the obstacle terms, after every other term: the
        // 24 link coordinates then live beside six finished terms and the end-effector position
        // instead of beside the record's tail and the kinematic sums.  The terms are added in
        // get_cost's order all the same.
        double t_joint = Cs.en_joint ? joint : 0.0, t_work = Cs.en_work ? wc : 0.0, t_energy = 0.0;
        if constexpr (EN) {   // energy_cost (:211-222)
            const double E = r[REC_E];
            t_energy = left_barrier(Cs.en_below, E) + right_barrier(Cs.en_above, E);
        }
        double t_vel = Cs.en_vel ? vel : 0.0;
        double t_traj = Cs.en_traj ? trajectory_term(Cs, sc, vl) : 0.0;
        double t_manip = Cs.en_manip ? manipulability_term(Cs, jj) : 0.0;
        double pe[3] = {ee[0], ee[1], ee[2]};
        int dep2 = 0;   // the (q, qd) reloads wait for those terms (an index, as above)
        asm volatile("" : "+v"(dep2), "+v"(pe[0]), "+v"(pe[1]), "+v"(pe[2]) : "v"(t_joint), "v"(t_work), "v"(t_energy), "v"(t_vel), "v"(t_traj), "v"(t_manip));
        const double *pq = reinterpret_cast<const double *>(tp + dep2);
        double qj[10], lp[SC_LINKS][3];
#pragma unroll
        for (int j = 0; j < 10; j++) qj[j] = lagged_q(pq[2 * j], pq[2 * j + 1], lm.dt, first);
        double R9[OB >= OB_TERM_HELD ? 9 : 1];   // body 9's rotation with the positions: the held object turns with the grasp
        if constexpr (OB >= OB_TERM_HELD) link_fk(*lm.model, qj, lp, R9);
        else link_fk(*lm.model, qj, lp);
        double sct = 0.0;
        if (Cs.en_self) sct = self_collision_term<false>(Cs, lp);
        double obt;
        if constexpr (OB >= OB_TERM_HELD) obt = obstacle_cost<OB>(ob, lp, pe, lm.dt, R9, lm.model->ee_R);
        else obt = obstacle_cost<OB>(ob, lp, pe, lm.dt);
        double cost = 0.0;
        cost += t_joint;
        cost += sct;
        cost += t_work;
        if constexpr (EN) cost += t_energy;
        cost += t_vel;
        cost += t_traj;
        cost += t_manip;
        cost += obt;
        return cost;
    }
    double cost = 0.0;
    cost += Cs.en_joint ? joint : 0.0;
    if constexpr (LP) {   // the (q, qd) pairs again, from the stored record (r holds its tail by now)
        double sct = 0.0;
        if (Cs.en_self) sct = record_self_collision<false>(Cs, *lm.model, reinterpret_cast<const double *>(tp), lm.dt, first);
        cost += sct;
    } else {
        cost += Cs.en_self ? Cs.self_collision : 0.0;
    }
    cost += Cs.en_work ? wc : 0.0;
    if constexpr (EN) {   // energy_cost (:211-222)
        const double E = r[REC_E];
        cost += left_barrier(Cs.en_below, E) + right_barrier(Cs.en_above, E);
    }
    cost += Cs.en_vel ? vel : 0.0;
    cost += Cs.en_traj ? trajectory_term(Cs, sc, vl) : 0.0;
    cost += Cs.en_manip ? manipulability_term(Cs, jj) : 0.0;
    return cost;
}

// The seven terms of AssistedManipulation::get_cost at one step record (the whole record in r), as
// the reference's per-term accumulators see them (assisted_manipulation.cpp:74-319: m_joint_cost
// += ..., read back by get_joint_limit_cost() .. get_manipulability_cost(), .hpp:232-258): joint
// limits, self-collision, workspace, energy, velocity, trajectory, manipulability; a disabled
// term is 0 (get_cost skips it).  Same arithmetic as assisted_manipulation_cost; the optimal
// rollout's totals only (mppi_optimal_terms) and the standalone get_cost, so off the rollout
// kernels' path.  yaw: dynamics->get_state()[2] (workspace_cost, :160-168; in a rollout the
// record's q_2).
// lp: the sphere links' positions (kinematic link-position model), or null: the zero stub's constant.
__device__ __forceinline__ void assisted_manipulation_terms(const DevCost &Cs, const StepConst &sc, const double *r, double yaw,
                                                            double *t, const double (*lp)[3] = nullptr)
{
    double j0 = 0.0, j1 = 0.0, v0 = 0.0, v1 = 0.0;
    for (int j = 0; j < FR_NB; j++) {
        const double q = r[REC_QQD + 2 * j], vq = fabs(r[REC_QQD + 2 * j + 1]);
        const double lj = left_barrier(Cs.lower[j], q) + right_barrier(Cs.upper[j], q);
        const double lv = Cs.vel_q[j] * (vq * vq);
        if (j < 6) { j0 += lj; v0 += lv; }
        else { j1 += lj; v1 += lv; }
    }
    double s, c;
    fsincos(yaw, &s, &c, sincos_constants());
    const double *ee = r + REC_EE, *am = r + REC_AM;
    double wc = 0.0;
    {
        const double r22 = (1.0 - c) + c;
        const double fw0 = c, fw1 = s, fw2 = 0.0;
        const double off0 = (0.1 * c + (-s) * 0.0) + 0.0 * 0.15;
        const double off1 = (0.1 * s + c * 0.0) + 0.0 * 0.15;
        const double off2 = (0.0 * 0.1 + 0.0 * 0.0) + r22 * 0.15;
        const double rb2 = am[2] + off2;
        const double t0 = ee[0] - (am[0] + off0), t1 = ee[1] - (am[1] + off1), t2 = ee[2] - rb2;
        const double proj = ((t0 * fw0 + t1 * fw1) + t2 * fw2) / ((fw0 * fw0 + fw1 * fw1) + fw2 * fw2);
        wc += left_barrier(Cs.ws_infront, proj);
        wc += right_barrier(Cs.ws_reach, sqrt((t0 * t0 + t1 * t1) + t2 * t2));
        const double n1 = sqrt(t0 * t0 + t1 * t1);
        const double n2 = sqrt(fw0 * fw0 + fw1 * fw1);
        const double ya = acos((t0 * fw0 + t1 * fw1) / n1 / n2);
        const double ay = fabs(ya);
        const double yc = (Cs.yaw_c + Cs.yaw_l * fabs(ay)) + Cs.yaw_q * ay * ay;
        wc += isnan(ya) ? 0.0 : yc;
        wc += left_barrier(Cs.ws_above, ee[2] - rb2);
    }
    const double E = r[REC_E];
    t[0] = Cs.en_joint ? j0 + j1 : 0.0;
    t[1] = Cs.en_self ? (lp ? self_collision_term<false>(Cs, lp) : Cs.self_collision) : 0.0;
    t[2] = Cs.en_work ? wc : 0.0;
    t[3] = Cs.en_energy ? left_barrier(Cs.en_below, E) + right_barrier(Cs.en_above, E) : 0.0;
    t[4] = Cs.en_vel ? v0 + v1 : 0.0;
    t[5] = Cs.en_traj ? trajectory_term(Cs, sc, r + REC_VL) : 0.0;
    t[6] = Cs.en_manip ? manipulability_term(Cs, r + REC_JJ) : 0.0;
}

// TrackPoint::get_cost: the joint terms sum joints 0..9 in order; reach_cost's robot point is the
// arm mount + R_z(yaw) (0.3, 0, 0.15) (track_point.cpp:162-186), yaw = dynamics->get_state()[2]
// (in a rollout the record's own q_2)
// LP: the self-collision term on the sphere links' positions lp (kinematic link-position model),
// else the zero stub's constant
// Target tracking (mppi_set_target_tracking): the step's target pose is tg (the StepConst seen as a
// StepTarget) when the wave-uniform Cs.tp_track is on, else the descriptor's point.  The orientation
// term w (3 - sum_ij Rt_ij Ree_ij) is added right behind the position term, before the joint,
// self-collision and reach terms: Rt the rotation of the target's unit quaternion, Ree = R9 ee_R with
// R9 body 9's world rotation at the lagged configuration of the link positions (link_fk).  A target
// without an orientation (the zero quaternion) contributes 0.
__device__ __forceinline__ double target_orientation_term(double w, double qx, double qy, double qz, double qw, const double *Ree)
{
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz;
    const double xw = qx * qw, yw = qy * qw, zw = qz * qw;
    const double Rt[9] = {1.0 - 2.0 * (yy + zz), 2.0 * (xy - zw),       2.0 * (xz + yw),
                          2.0 * (xy + zw),       1.0 - 2.0 * (xx + zz), 2.0 * (yz - xw),
                          2.0 * (xz - yw),       2.0 * (yz + xw),       1.0 - 2.0 * (xx + yy)};
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) s += Rt[k] * Ree[k];
    const double n2 = (xx + yy) + (zz + qw * qw);
    return (n2 == 0.0) ? 0.0 : w * (3.0 - s);
}
// Ree = R9 ee_R (row-major)
__device__ __forceinline__ void grasp_rotation(const double *R9, const double *eeR, double *Ree)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) Ree[3 * r + c] = (R9[3 * r] * eeR[c] + R9[3 * r + 1] * eeR[3 + c]) + R9[3 * r + 2] * eeR[6 + c];
    }
}

// The step's orientation term from body 9's rotation, formed where link_fk leaves R9 so that the
// rotation is dead again before the other terms run (held across them, the obstacle units spilled)
__device__ __forceinline__ double step_orientation_term(const DevCost &Cs, const StepTarget *tg, const double *R9, const DevModel &M)
{
    // row by row, each row's sum finished before the next begins: three entries of Rt and of Ree live
    // at a time instead of eighteen beside the record and the link positions
    const double qx = tg->q[0], qy = tg->q[1], qz = tg->q[2], qw = tg->qw;
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double t0, t1, t2;
        if (i == 0) { t0 = 1.0 - 2.0 * (yy + zz); t1 = 2.0 * (qx * qy - qz * qw); t2 = 2.0 * (qx * qz + qy * qw); }
        else if (i == 1) { t0 = 2.0 * (qx * qy + qz * qw); t1 = 1.0 - 2.0 * (xx + zz); t2 = 2.0 * (qy * qz - qx * qw); }
        else { t0 = 2.0 * (qx * qz - qy * qw); t1 = 2.0 * (qy * qz + qx * qw); t2 = 1.0 - 2.0 * (xx + yy); }
        const double *R = R9 + 3 * i, *E = M.ee_R;
        const double e0 = (R[0] * E[0] + R[1] * E[3]) + R[2] * E[6];
        const double e1 = (R[0] * E[1] + R[1] * E[4]) + R[2] * E[7];
        const double e2 = (R[0] * E[2] + R[1] * E[5]) + R[2] * E[8];
        s += (t0 * e0 + t1 * e1) + t2 * e2;
        asm volatile("" : "+v"(s));
    }
    const double n2 = (xx + yy) + (zz + qw * qw);
    return (n2 == 0.0) ? 0.0 : Cs.tp_orient_w * (3.0 - s);
}

// The orientation term of a stored step record, as a function that is called, not inlined: it reads
// the record's (q, qd) pairs again from memory and runs a pass of link_fk of its own, whose positions
// nobody reads (the compiler drops them: the rotation chain alone).  Inlined into the objective - from
// the terms' own link_fk pass or from a pass of its own - it cost every LP unit's TrackPoint kernels
// 84 to 690 bytes of scratch per lane, spilled in the kernels' prologues whether the handle tracks or
// not; called, its registers are saved and restored around the call, inside the wave-uniform branch
// of a tracking handle, and the rollout units hold one copy of it each.
static __device__ __attribute__((noinline)) double record_orientation_term(const double2 *src, const StepTarget *tg, const DevModel *M,
                                                                  const DevCost *Cs, double dt, bool first)
{
    double qj[10], lpr[SC_LINKS][3], R9[9];
#pragma unroll
    for (int j = 0; j < 10; j++) {
        const double2 v = src[j];
        qj[j] = lagged_q(v.x, v.y, dt, first);
    }
    link_fk(*M, qj, lpr, R9);
    return step_orientation_term(*Cs, tg, R9, *M);
}

// tg: a rollout's step (its target behind Cs.tp_track), orient its orientation term (behind
// Cs.tp_track_orient); the device object's get_cost passes neither and reads the descriptor's point
template <bool LP = false>
__device__ __forceinline__ double track_point_cost(const DevCost &Cs, const double *r, double yaw, const double (*lp)[3] = nullptr,
                                                   const StepTarget *tg = nullptr, double orient = 0.0)
{
    const double *ee = r + REC_EE, *am = r + REC_AM;
    double g0 = Cs.tp_point[0], g1 = Cs.tp_point[1], g2 = Cs.tp_point[2];
    const bool track = tg != nullptr && Cs.tp_track != 0;
    if (track) {
        g0 = tg->p[0];
        g1 = tg->p[1];
        g2 = tg->p[2];
    }
    const double d0 = ee[0] - g0, d1 = ee[1] - g1, d2 = ee[2] - g2;
    const double distance = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    double cost = 100.0 * (distance * distance);   // point_cost: 100 pow(distance, 2)
    if constexpr (LP) {
        if (track && Cs.tp_track_orient) cost += orient;
    }
    double joint = 0.0;
#pragma unroll
    for (int j = 0; j < 10; j++) {
        const double q = r[REC_QQD + 2 * j], lo = Cs.tp_lo[j], up = Cs.tp_up[j];
        const double below = (q < lo) ? 1000.0 + 100000.0 * ((lo - q) * (lo - q)) : 0.0;
        const double above = (q > up) ? 1000.0 + 100000.0 * ((q - up) * (q - up)) : 0.0;
        joint += below + above;
    }
    double s, c;
    fsincos(yaw, &s, &c, sincos_constants());
    const double r22 = (1.0 - c) + c;
    const double off0 = (0.3 * c + (-s) * 0.0) + 0.0 * 0.15;
    const double off1 = (0.3 * s + c * 0.0) + 0.0 * 0.15;
    const double off2 = (0.0 * 0.3 + 0.0 * 0.0) + r22 * 0.15;
    const double t0 = ee[0] - (am[0] + off0), t1 = ee[1] - (am[1] + off1), t2 = ee[2] - (am[2] + off2);
    const double reach = right_barrier(Cs.tp_reach, sqrt((t0 * t0 + t1 * t1) + t2 * t2));
    cost += Cs.tp_en_joint ? joint : 0.0;
    if constexpr (LP) {
        double sct = 0.0;
        if (Cs.tp_en_self) sct = self_collision_term<true>(Cs, lp);
        cost += sct;
    } else {
        cost += Cs.tp_en_self ? Cs.tp_self : 0.0;
    }
    cost += Cs.tp_en_reach ? reach : 0.0;
    return cost;
}

__device__ __forceinline__ double readlane_f64(double x, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}

// gamma_k times the objective at step record r (AssistedManipulation: r holds the record's (q, qd)
// pairs, the rest is read from the stored record src; TrackPoint: r holds the record up to REC_VL)
template <int CK, bool EN, int JS = JT_STRIDE, bool KC = false, int JG = 1, bool LP = false, int OB = OB_TERM_NONE>
__device__ __forceinline__ double step_cost(const DevCost &Cs, const StepConst &sc, const double *r, const double *Lj,
                                           const double2 *src, LinkModel lm = LinkModel{}, bool first = false,
                                           ObstacleRef ob = ObstacleRef{})
{
    if constexpr (CK == CK_TRACK_POINT) {
        // (a tracking handle's step constants hold the step's target: engine_types.hpp StepTarget)
        const StepTarget *tg = reinterpret_cast<const StepTarget *>(&sc);
        if constexpr (LP) {
            double orient = 0.0;
            if (Cs.tp_track_orient) orient = record_orientation_term(src, tg, lm.model, &Cs, lm.dt, first);
            double lp[SC_LINKS][3];
            if constexpr (OB >= OB_TERM_HELD) {   // the held object turns with the grasp: body 9's rotation with the positions
                double qj[10], R9[9];
#pragma unroll
                for (int j = 0; j < 10; j++) qj[j] = lagged_q(r[REC_QQD + 2 * j], r[REC_QQD + 2 * j + 1], lm.dt, first);
                link_fk(*lm.model, qj, lp, R9);
                return sc.gamma_k * (track_point_cost<true>(Cs, r, r[REC_QQD + 4], lp, tg, orient) +
                                     obstacle_cost<OB>(ob, lp, r + REC_EE, lm.dt, R9, lm.model->ee_R));
            }
            if (Cs.tp_en_self || OB) {
                double qj[10];
#pragma unroll
                for (int j = 0; j < 10; j++) qj[j] = lagged_q(r[REC_QQD + 2 * j], r[REC_QQD + 2 * j + 1], lm.dt, first);
                link_fk(*lm.model, qj, lp);
            }
            if constexpr (OB)
                return sc.gamma_k * (track_point_cost<true>(Cs, r, r[REC_QQD + 4], lp, tg, orient) +
                                     obstacle_cost<OB>(ob, lp, r + REC_EE, lm.dt));
            else
                return sc.gamma_k * track_point_cost<true>(Cs, r, r[REC_QQD + 4], lp, tg, orient);
        } else {
            return sc.gamma_k * track_point_cost(Cs, r, r[REC_QQD + 4], nullptr, tg);
        }
    } else {
        if constexpr (OB) return sc.gamma_k * assisted_manipulation_cost<EN, JS, KC, JG, true, OB>(Cs, sc, r, Lj, src, lm, first, ob);
        else if constexpr (LP) return sc.gamma_k * assisted_manipulation_cost<EN, JS, KC, JG, true>(Cs, sc, r, Lj, src, lm, first);
        else return sc.gamma_k * assisted_manipulation_cost<EN, JS, KC, JG>(Cs, sc, r, Lj, src);
    }
}

// gamma_k times the objective at the stored step record rk (FR_REC doubles, or FR_REC_C with KC;
// 16-byte aligned)
template <int CK, bool EN, int JS = JT_STRIDE, bool KC = false, int JG = 1, bool LP = false, int OB = OB_TERM_NONE>
__device__ __forceinline__ double record_step_cost(const DevCost &Cs, const StepConst &sc, const double *rk, const double *Lj,
                                                  LinkModel lm = LinkModel{}, bool first = false, ObstacleRef ob = ObstacleRef{})
{
    double r[FR_NREC];
    const double2 *src = reinterpret_cast<const double2 *>(rk);
    constexpr int NLOAD = CK == CK_TRACK_POINT ? REC_VL / 2 : FR_NB;   // AssistedManipulation: the (q, qd) pairs
#pragma unroll
    for (int i = 0; i < NLOAD; i++) {
        const double2 v = src[i];
        r[2 * i] = v.x;
        r[2 * i + 1] = v.y;
    }
    if constexpr (OB) return step_cost<CK, EN, JS, KC, JG, true, OB>(Cs, sc, r, Lj, src, lm, first, ob);
    else if constexpr (LP) return step_cost<CK, EN, JS, KC, JG, true>(Cs, sc, r, Lj, src, lm, first);
    else return step_cost<CK, EN, JS, KC, JG>(Cs, sc, r, Lj, src);
}

// J of one rollout from its H stored step records (rollout-major, FR_REC doubles each, FR_REC_C with
// KC) by one wave:
// lane k evaluates step k (64 steps a pass) and the wave sums the step costs in step order, as the
// reference accumulates J += cost (mppi.cpp:322-337); a NaN step makes the sum NaN (the reference's
// early stop), canonicalised to the quiet NaN it stores.  The same value on every lane.
// OB: the obstacle term from the table behind stp (one row a wave: one table)
template <int CK, bool EN, int JS = JT_STRIDE, bool KC = false, bool LP = false, int OB = OB_TERM_NONE>
__device__ __forceinline__ double rollout_cost(const DevCost &Cs, const StepConst *stp, const double *rec, int H, int lane,
                                               const double *Lj, LinkModel lm = LinkModel{})
{
    constexpr int RS = KC ? FR_REC_C : FR_REC;
    double J = 0.0;
    for (int base = 0; base < H; base += 64) {
        const int n = (H - base < 64) ? H - base : 64;
        const int k = base + (lane < n ? lane : 0);
        double c;
        if constexpr (OB)
            c = record_step_cost<CK, EN, JS, KC, 1, true, OB>(Cs, stp[k], rec + (int64_t)k * RS, Lj, lm, k == 0,
                                                                ObstacleRef{obstacle_table_of(stp, H), nullptr, false, k});
        else if constexpr (LP) c = record_step_cost<CK, EN, JS, KC, 1, true>(Cs, stp[k], rec + (int64_t)k * RS, Lj, lm, k == 0);
        else c = record_step_cost<CK, EN, JS, KC>(Cs, stp[k], rec + (int64_t)k * RS, Lj);
        // J += c_i in step order; the lane reads eight at a time, ahead of their adds
        int i = 0;
        for (; i + 8 <= n; i += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = readlane_f64(c, i + u);
#pragma unroll
            for (int u = 0; u < 8; u++) J += v[u];
        }
        for (; i < n; i++) J += readlane_f64(c, i);
    }
    return isnan(J) ? (double)NAN : J;
}

// The costs' min / max / count (CostStats) gain one cost (NaN ones are not counted), in the slot
// of its rollout index
__device__ __forceinline__ void fold_cost_stats(CostStats *st, double J, int64_t r)
{
    if (!st || isnan(J)) return;
    const unsigned long long key = mppi_dev::cost_order_key(J);
    const int i = (int)(r & (CS_SLOTS - 1));
    atomicMin(&st->kmin[16 * i], key);
    atomicMax(&st->kmax[16 * i], key);
    atomicAdd(&st->count[32 * i], 1u);
}

}  // namespace mppi_cost
