// fr_safety.hip — the trajectory safety filter on the device: joint position, velocity and
// acceleration limits applied to the plan U* between the finish kernel and the publish
// (FrankaRidgeback::TrajectorySafetyFilter, whose bodies the reference leaves empty; the
// definition is DESIGN.md §1 "Safety filter").
//
// One workgroup of one wave walks the H steps of the plan from the update's x0.  The kernel sits
// on the update's critical path, so a step is spread over the wave instead of run by one thread:
//   - lane p < 12 owns joint j = PERM[p] (its q, v, limits and body constants in registers); the
//     order (0, 1, 2, 10, 11, 3 .. 9) puts the joints whose torque the filter leaves alone first;
//   - the kinematic chain's rows are independent (row r of R_i reads row r of R_parent only), so
//     three lanes carry one row each through the twelve bodies without a hand-off;
//   - the 144 entries of the composite-inertia matrix are one dot product each, three per lane;
//   - the solve is a Gaussian elimination with row p of the permuted matrix in lane p's registers
//     and the pivot row broadcast by v_readlane (no LDS, no pivoting: M is symmetric positive
//     definite).  After the five pivots of B = {0, 1, 2, 10, 11} the remaining 7x7 block IS the
//     Schur complement M_AA - M_AB M_BB^-1 M_BA of the arm joints A, and the five finished rows
//     are the factor of M_BB: the arm correction du_A = S da_A and the coupled da_B (U_BB da_B =
//     -U_BA da_A) fall out of the one elimination that also gives a = M^-1 tau.
// U* (H x 12), the wrench rows and each lane's body are staged once; the step loop touches LDS and
// registers only; the filtered plan, the forwarded status words and the sequence flag are written
// at the end with the finish kernels' store discipline (kernels.hip publish_block).
//
// The second kernel filters one column at a dynamics object's (q, v) with the same step function.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "device_common.hpp"
#include "engine_types.hpp"
#include "kernels.hpp"
#include "fsincos.hpp"

using namespace mppi_eng;
using mppi_dev::smax;
using mppi_dev::smin;

namespace {

// per-step scratch in LDS, doubles
struct StepLds {
    double Rl[FR_NB][9], pl[FR_NB][3];   // joint placements in the parent frame at q
    double Rw[FR_NB][9], pw[FR_NB][3];   // world placements
    double S[FR_NB][6], F[FR_NB][6];     // motion subspaces, composite inertia times them
    double comp[FR_NB][10];              // composite (m, h[3], I[6] about the origin: xx xy xz yy yz zz)
    double M[FR_NB][FR_NB];              // the mass matrix in the lanes' joint order
};

// lane -> joint: B = {0, 1, 2, 10, 11} first, then the arm 3 .. 9
__device__ __forceinline__ int perm(int p) { return p < 3 ? p : (p < 5 ? p + 7 : p - 2); }

__device__ __forceinline__ double bc(double v, int lane)   // lane is wave-uniform
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// 1 / x: v_rcp_f64 and two Newton steps (the quotient's last bits are below the solve's own rounding)
__device__ __forceinline__ double rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    return __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
}

__device__ __forceinline__ void cross3(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot6(const double *a, const double *b)
{
    return ((a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3])) + (a[4] * b[4] + a[5] * b[5]);
}

// one joint's constants and limits, in its lane's registers
struct LaneJoint {
    int j, kind;            // joint and its JointKind
    double R[9], p[3], mass, c[3], Ic[6];
    double pmin, pmax, vmin, vmax, amin, amax;
};

__device__ __forceinline__ void load_lane(const DevModel &M, const SafetyLimits &L, int lane, LaneJoint &J)
{
    const int p = lane < FR_NB ? lane : FR_NB - 1;   // the idle lanes mirror the last joint (never stored)
    const int j = perm(p);
    J.j = j;
    J.kind = j == 0 ? KIND_PX : (j == 1 || j == 10) ? KIND_PY : j == 11 ? KIND_PNY : KIND_RZ;
    const DevBody &b = M.b[j];
    for (int k = 0; k < 9; k++) J.R[k] = b.R[k];
    for (int k = 0; k < 3; k++) { J.p[k] = b.p[k]; J.c[k] = b.c[k]; }
    for (int k = 0; k < 6; k++) J.Ic[k] = b.Ic[k];
    J.mass = b.mass;
    J.pmin = L.position_minimum[j]; J.pmax = L.position_maximum[j];
    J.vmin = L.velocity_minimum[j]; J.vmax = L.velocity_maximum[j];
    J.amin = L.acceleration_minimum[j]; J.amax = L.acceleration_maximum[j];
}

// clampseq of DESIGN §1: position, velocity, acceleration, a later clamp wins
__device__ __forceinline__ double clampseq(const LaneJoint &J, const SafetyLimits &L, double x, double q, double v, double dt)
{
    if (L.limit_joints) x = smin(smax(x, (J.pmin - q) / dt), (J.pmax - q) / dt);
    if (L.limit_velocity) x = smin(smax(x, J.vmin), J.vmax);
    if (L.limit_acceleration) x = smin(smax(x, v + J.amin * dt), v + J.amax * dt);
    return x;
}

// One step of the filter for the whole wave.  In: the lane's joint state (q, v) and control u, the
// step's wrench (or null).  Out: the filtered control u and the state after the dynamics' step under
// it.  Returns whether the filter changed the column (wave-uniform).
__device__ __forceinline__ bool safety_step(StepLds &W, const DevModel &M, const SafetyLimits &L, const LaneJoint &J, int lane,
                                            double &q, double &v, double &u, const double *w, double dt)
{
    const bool on = lane < FR_NB;
    const int j = J.j;
    // P1: the joint's placement at q
    double sq, cq;   // (the rollout kernels' branch-free sincos; every lane, the prismatic joints' unused)
    fsincos(q, &sq, &cq, SinCosK{{-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04,
                                  2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10},
                                 {4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05,
                                  -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11}});
    if (on) {
        double *Rl = W.Rl[j], *pl = W.pl[j];
        if (J.kind == KIND_RZ) {
            for (int r = 0; r < 3; r++) {
                Rl[3 * r + 0] = J.R[3 * r + 0] * cq + J.R[3 * r + 1] * sq;
                Rl[3 * r + 1] = J.R[3 * r + 0] * (-sq) + J.R[3 * r + 1] * cq;
                Rl[3 * r + 2] = J.R[3 * r + 2];
                pl[r] = J.p[r];
            }
        } else {
            const int col = J.kind == KIND_PX ? 0 : 1;
            const double qq = J.kind == KIND_PNY ? -q : q;
            for (int r = 0; r < 3; r++) {
                for (int k = 0; k < 3; k++) Rl[3 * r + k] = J.R[3 * r + k];
                pl[r] = J.p[r] + J.R[3 * r + col] * qq;
            }
        }
    }
    __syncthreads();
    // P2: the chain, one row of every world placement per lane (lanes 0..2); bodies 10 and 11 both hang off 9
    if (lane < 3) {
        double row[3] = {lane == 0 ? 1.0 : 0.0, lane == 1 ? 1.0 : 0.0, lane == 2 ? 1.0 : 0.0}, pr = 0.0;
        double row9[3] = {0, 0, 0}, pr9 = 0.0;
        // four bodies at a time: their placements loaded together (one LDS round trip, not one per
        // operand behind the previous body's stores), the chain in registers, the rows stored after
#pragma unroll
        for (int i0 = 0; i0 < FR_NB; i0 += 4) {
            double Rl[4][9], pl[4][3], o[4][4];
#pragma unroll
            for (int b = 0; b < 4; b++) {
#pragma unroll
                for (int k = 0; k < 9; k++) Rl[b][k] = W.Rl[i0 + b][k];
#pragma unroll
                for (int k = 0; k < 3; k++) pl[b][k] = W.pl[i0 + b][k];
            }
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int i = i0 + b;
                if (i == 11) { row[0] = row9[0]; row[1] = row9[1]; row[2] = row9[2]; pr = pr9; }
                const double n0 = (row[0] * Rl[b][0] + row[1] * Rl[b][3]) + row[2] * Rl[b][6];
                const double n1 = (row[0] * Rl[b][1] + row[1] * Rl[b][4]) + row[2] * Rl[b][7];
                const double n2 = (row[0] * Rl[b][2] + row[1] * Rl[b][5]) + row[2] * Rl[b][8];
                pr = pr + ((row[0] * pl[b][0] + row[1] * pl[b][1]) + row[2] * pl[b][2]);
                row[0] = n0; row[1] = n1; row[2] = n2;
                o[b][0] = n0; o[b][1] = n1; o[b][2] = n2; o[b][3] = pr;
                if (i == 9) { row9[0] = n0; row9[1] = n1; row9[2] = n2; pr9 = pr; }
            }
#pragma unroll
            for (int b = 0; b < 4; b++) {
                W.Rw[i0 + b][3 * lane + 0] = o[b][0]; W.Rw[i0 + b][3 * lane + 1] = o[b][1]; W.Rw[i0 + b][3 * lane + 2] = o[b][2];
                W.pw[i0 + b][lane] = o[b][3];
            }
        }
    }
    __syncthreads();
    // P3: the joint's motion subspace and its body's own inertia about the origin
    double S[6] = {0, 0, 0, 0, 0, 0};
    if (on) {
        double R[9], p[3];
        for (int k = 0; k < 9; k++) R[k] = W.Rw[j][k];
        for (int k = 0; k < 3; k++) p[k] = W.pw[j][k];
        if (J.kind == KIND_RZ) {
            const double ax[3] = {R[2], R[5], R[8]};
            cross3(p, ax, S);
            S[3] = ax[0]; S[4] = ax[1]; S[5] = ax[2];
        } else {
            const int col = J.kind == KIND_PX ? 0 : 1;
            const double sg = J.kind == KIND_PNY ? -1.0 : 1.0;
            S[0] = sg * R[col]; S[1] = sg * R[3 + col]; S[2] = sg * R[6 + col];
        }
        for (int k = 0; k < 6; k++) W.S[j][k] = S[k];
        double c[3];
        for (int r = 0; r < 3; r++) c[r] = ((R[3 * r] * J.c[0] + R[3 * r + 1] * J.c[1]) + R[3 * r + 2] * J.c[2]) + p[r];
        const double I[9] = {J.Ic[0], J.Ic[1], J.Ic[3], J.Ic[1], J.Ic[2], J.Ic[4], J.Ic[3], J.Ic[4], J.Ic[5]};
        double RI[9], Iw[6];
        for (int r = 0; r < 3; r++)
            for (int cc = 0; cc < 3; cc++) RI[3 * r + cc] = (R[3 * r] * I[cc] + R[3 * r + 1] * I[3 + cc]) + R[3 * r + 2] * I[6 + cc];
        int n = 0;
        for (int r = 0; r < 3; r++)
            for (int cc = r; cc < 3; cc++, n++) Iw[n] = (RI[3 * r] * R[3 * cc] + RI[3 * r + 1] * R[3 * cc + 1]) + RI[3 * r + 2] * R[3 * cc + 2];
        const double mi = J.mass, cc2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
        double *o = W.comp[j];
        o[0] = mi;
        for (int k = 0; k < 3; k++) o[1 + k] = mi * c[k];
        o[4] = Iw[0] + mi * (cc2 - c[0] * c[0]);
        o[5] = Iw[1] - mi * c[0] * c[1];
        o[6] = Iw[2] - mi * c[0] * c[2];
        o[7] = Iw[3] + mi * (cc2 - c[1] * c[1]);
        o[8] = Iw[4] - mi * c[1] * c[2];
        o[9] = Iw[5] + mi * (cc2 - c[2] * c[2]);
    }
    __syncthreads();
    // P4: children into parents, one of the ten composite quantities per lane
    if (lane < 10) {
        double c[FR_NB];   // twelve independent loads, then the sums in registers
#pragma unroll
        for (int i = 0; i < FR_NB; i++) c[i] = W.comp[i][lane];
        c[9] += c[11];
#pragma unroll
        for (int i = 10; i > 0; i--) c[i == 10 ? 9 : i - 1] += c[i];
#pragma unroll
        for (int i = 0; i < 10; i++) W.comp[i][lane] = c[i];
    }
    __syncthreads();
    // P5: F_j = Ic_j S_j = [m v - h x w; h x v + I w]; the wrench's joint torque S_j . (f, m + p_ee x f)
    double tau = (on && j >= FR_ARM0 && j < FR_ARM1) ? u : 0.0;
    if (on) {
        const double *cm = W.comp[j];
        const double h[3] = {cm[1], cm[2], cm[3]};
        double hw[3], hv[3];
        cross3(h, S + 3, hw);
        cross3(h, S, hv);
        double *F = W.F[j];
        for (int k = 0; k < 3; k++) F[k] = cm[0] * S[k] - hw[k];
        F[3] = hv[0] + ((cm[4] * S[3] + cm[5] * S[4]) + cm[6] * S[5]);
        F[4] = hv[1] + ((cm[5] * S[3] + cm[7] * S[4]) + cm[8] * S[5]);
        F[5] = hv[2] + ((cm[6] * S[3] + cm[8] * S[4]) + cm[9] * S[5]);
        if (w && j <= FR_EE_PARENT) {
            const double *R9 = W.Rw[FR_EE_PARENT], *p9 = W.pw[FR_EE_PARENT];
            double pe[3], mo[3];
            for (int r = 0; r < 3; r++) pe[r] = p9[r] + ((R9[3 * r] * M.ee_p[0] + R9[3 * r + 1] * M.ee_p[1]) + R9[3 * r + 2] * M.ee_p[2]);
            cross3(pe, w, mo);
            for (int r = 0; r < 3; r++) mo[r] = w[3 + r] + mo[r];
            tau += ((S[0] * w[0] + S[1] * w[1]) + S[2] * w[2]) + ((S[3] * mo[0] + S[4] * mo[1]) + S[5] * mo[2]);
        }
    }
    __syncthreads();
    // P6: M[i][j] = S_i . F_j for i on j's path to the root (the fingers are siblings), symmetric
#pragma unroll
    for (int e = lane; e < FR_NB * FR_NB; e += 64) {
        const int pr = e / FR_NB, pc = e - pr * FR_NB;
        const int a = perm(pr), b = perm(pc);
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        W.M[pr][pc] = (lo == 10 && hi == 11) ? 0.0 : dot6(W.S[lo], W.F[hi]);
    }
    __syncthreads();
    // P7: the elimination, row p in lane p
    const int p = lane < FR_NB ? lane : FR_NB - 1;
    double row[FR_NB], inv[FR_NB], Sc[7];
#pragma unroll
    for (int k = 0; k < FR_NB; k++) row[k] = W.M[p][k];
    double y = tau;
#pragma unroll
    for (int k = 0; k < FR_NB; k++) {
        inv[k] = rcp(bc(row[k], k));
        const double f = lane > k ? row[k] * inv[k] : 0.0;   // (the rows above the pivot are finished)
#pragma unroll
        for (int c = k + 1; c < FR_NB; c++) row[c] -= f * bc(row[c], k);
        y -= f * bc(y, k);
        if (k == 4) {
#pragma unroll
            for (int c = 0; c < 7; c++) Sc[c] = row[5 + c];   // the arm rows' Schur complement
        }
    }
    double a = 0.0;
#pragma unroll
    for (int k = FR_NB - 1; k >= 0; k--) {
        const double xk = bc(y, k) * inv[k];
        if (lane == k) a = xk;
        if (lane < k) y -= row[k] * xk;
    }
    // the step: base velocity in world axes, the unfiltered next velocity
    const double spsi = bc(sq, 2), cpsi = bc(cq, 2);
    const double u0 = bc(u, 0), u1 = bc(u, 1), u2 = bc(u, 2);
    const bool base = lane < 3, arm = lane >= 5 && lane < FR_NB;
    double wv = lane == 0 ? cpsi * u0 + (-spsi) * u1 : lane == 1 ? spsi * u0 + cpsi * u1 : u2;
    const double vc = base ? wv : v;
    const double vplus = vc + a * dt;
    // the arm's limits: the change of acceleration that meets them, the arm torque that makes it
    double da = 0.0;
    if (arm) {
        const double t = clampseq(J, L, vplus, q, v, dt);
        if (t != vplus) da = (t - vplus) / dt;
    }
    const bool any_arm = __ballot(da != 0.0) != 0ull;
    if (any_arm) {
        double du = 0.0, acc = 0.0;
#pragma unroll
        for (int c = 5; c < FR_NB; c++) {
            const double dc = bc(da, c);
            du += Sc[c - 5] * dc;
            acc -= row[c] * dc;   // lanes 0..4: -U_BA da_A
        }
        double dab = 0.0;
#pragma unroll
        for (int k = 4; k >= 0; k--) {
            const double xk = bc(acc, k) * inv[k];
            if (lane == k) dab = xk;
            if (lane < k) acc -= row[k] * xk;
        }
        if (arm) { u += du; a += da; }
        else if (lane < 5) a += dab;
    }
    // the base's limits on the velocity it would have after the arm's correction
    double dw = 0.0;
    if (base) {
        const double vp = wv + a * dt;
        dw = clampseq(J, L, vp, q, v, dt) - vp;
    }
    const bool any_base = __ballot(dw != 0.0) != 0ull;
    if (any_base) {
        const double d0 = bc(dw, 0), d1 = bc(dw, 1), d2 = bc(dw, 2);
        if (lane == 0) u += cpsi * d0 + spsi * d1;
        if (lane == 1) u += (-spsi) * d0 + cpsi * d1;
        if (lane == 2) u += d2;
        wv += dw;
    }
    // the dynamics' step under the filtered control (pinocchio_dynamics.cpp:226-260)
    v = (base ? wv : v) + a * dt;
    q = q + v * dt;
    __syncthreads();   // the scratch is rewritten by the next step
    return any_arm || any_base;
}

__device__ __forceinline__ void pub(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

}  // namespace

__global__ __launch_bounds__(64) void fr_safety_filter_kernel(SafetyArgs a)
{
    extern __shared__ double lds[];
    StepLds &W = *reinterpret_cast<StepLds *>(lds);
    double *Ul = lds + sizeof(StepLds) / sizeof(double);   // [H][12]
    double *Wl = Ul + a.H * FR_C;                          // [H][6]
    const int lane = threadIdx.x, HC = a.H * FR_C;
    const double *st = a.stage + HC;
    // the finish kernel did not publish a new plan (all-NaN, smoothing error, wait timeouts): forward
    const bool forward = st[1] != 0.0 || st[3] != 0.0 || st[7] != 0.0;
    for (int t = lane; t < HC; t += 64) Ul[t] = a.stage[t];
    if (a.wrench)
        for (int t = lane; t < a.H * 6; t += 64) Wl[t] = a.wrench[(t / 6) * FR_WRENCH_ROW + t % 6];
    LaneJoint J;
    load_lane(*a.model, a.lim, lane, J);
    double q = a.x0[J.j], v = a.x0[FR_NB + J.j];
    __syncthreads();
    int changed = 0;
    if (!forward) {
        for (int k = 0; k < a.H; k++) {
            double u = Ul[k * FR_C + J.j];
            const bool ch = safety_step(W, *a.model, a.lim, J, lane, q, v, u, a.wrench ? Wl + 6 * k : nullptr, a.dt);
            if (ch) {
                if (lane < FR_NB) Ul[k * FR_C + J.j] = u;
                changed++;
            }
        }
        __syncthreads();
    }
    for (int t = lane; t < HC; t += 64) {
        const double val = Ul[t];
        if (!forward) a.U[t] = val;
        pub(a.out + t, val);
    }
    if (lane < 8 && lane != 6) pub(a.out + HC + lane, st[lane]);
    if (lane == 8) pub(a.out + HC + 8, (double)changed);
    // every lane's block stores acknowledged, then the sequence flag (kernels.hip publish_block)
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (lane == 0) __hip_atomic_store(a.out + HC + 6, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// mppi_dynamics_safety_filter: one column at the object's current (q, v)
__global__ __launch_bounds__(64) void fr_safety_column_kernel(const DevPinocchio *obj, const DevModel *model, SafetyLimits lim,
                                                              SafetyColumn c, double *out12)
{
    __shared__ StepLds W;
    const int lane = threadIdx.x;
    LaneJoint J;
    load_lane(*model, lim, lane, J);
    double q = obj->q[J.j], v = obj->v[J.j], u = c.u[J.j];
    safety_step(W, *model, lim, J, lane, q, v, u, c.has_wrench ? c.w : nullptr, c.dt);
    if (lane < FR_NB) out12[J.j] = u;
}

namespace mppi_eng {

size_t fr_safety_lds_bytes(int H) { return sizeof(StepLds) + (size_t)H * (FR_C + 6) * sizeof(double); }

hipError_t launch_fr_safety_filter(const SafetyArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(fr_safety_filter_kernel, dim3(1), dim3(64), fr_safety_lds_bytes(a.H), s, a);
    return hipGetLastError();
}

hipError_t launch_fr_safety_column(const DevPinocchio *obj, const DevModel *model, const SafetyLimits &lim, const SafetyColumn &c,
                                   double *out12, hipStream_t s)
{
    hipLaunchKernelGGL(fr_safety_column_kernel, dim3(1), dim3(64), 0, s, obj, model, lim, c, out12);
    return hipGetLastError();
}

}  // namespace mppi_eng
