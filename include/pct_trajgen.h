/* pct_trajgen.h -- C ABI of the trajectory generator (libpct_engine.so): a chain of free spheres and a time allocation in, a
 * minimum-jerk piecewise Bezier trajectory inside the spheres out, B candidates per call.
 *
 * The step of the reference between the corridor finder and the checks: trajGeneration's timeAllocation
 * (Planner/src/sim_planning_demo.cpp:603-686) and BezierConicOptimizer (Planner/src/traj_optimizer.cpp:24-760).  The reference
 * hands the problem to a closed-source conic solver; the problem itself is restated here and solved by ADMM, one workgroup per
 * candidate, so that one corridor can be solved under several time allocations at once and the results go straight into
 * pct_bezier_check_batch_dev / pct_bezier_certify_batch_dev (include/pct_engine.h) on the same device buffers.
 *
 * Trajectory generation (pct_bezier_generate_batch*): the contract.
 *
 * The problem.  Candidate b owns segments [seg_offsets[b], seg_offsets[b+1]), m = 1..16 of them.  Segment i has order n_i (5..12),
 * duration T_i and control points P_i0..P_in in world units (metres); the unknown x stacks them, N = sum(n_i + 1) <= 208 per axis.
 * Objective: the integral of the squared k-th derivative (k = minimize_order) over the whole trajectory, summed over the axes,
 *     cost = 1/2 x^T P x per axis,  P = blockdiag_i(2 * T_i^(1-2k) * M_k(n_i)),  M_k(n) = f^2 * D_k^T * G * D_k,
 * D_k the k-fold forward difference, f = n!/(n-k)!, G[a][b] = C(q,a) * C(q,b) / C(2q,a+b) / (2q+1), q = n - k (the Gram matrix of
 * the Bernstein basis).  This is the reference's objective with its T-scaling T^((2k-3)/2) on coef = P/T (traj_optimizer.cpp:527).
 * Rows of E (equalities, kept exact; per axis 3 at the start, 3 at the end and 3 per joint = 9 start, 9 end and 9 per joint over
 * the axes, as traj_optimizer.cpp:263-445), in differences of control points d1 = P_(j+1) - P_j, d2 = P_(j+2) - 2 P_(j+1) + P_j:
 *     start:  P_00 = p,  d1 = v * T_0/n_0,  d2 = a * T_0^2/(n_0 (n_0 - 1))         end: the same on the last three points
 *     joint between segments i and i+1:  P_in = P_(i+1)0,  d1_last(i) = g1 * d1_first(i+1),  d2_last(i) = g2 * d2_first(i+1),
 *     g1 = (n'/T') * (T/n),  g2 = (n'(n'-1)/T'^2) * (T^2/(n(n-1)))   (velocity and acceleration continuous: C2 joints)
 * Rows of Gv and Ga (inequalities): every first difference of a segment, |d1| <= max_vel * T_i/n_i, and every second difference,
 * |d2| <= max_acc * T_i^2/(n_i (n_i - 1)), per axis -- the velocity and acceleration control values bounded, in metres.  A limit
 * <= 0 or +inf drops its rows.  Balls: every control point of segment i inside the sphere (centre_i, radius_i - margin).
 *
 * The algorithm.  ADMM on  min 1/2 x^T Q x  s.t.  E x = b,  z = A x,  z in C,  Q = P / max|P| (so max|Q| = 1), A = [I; Gv; Ga],
 * C = balls x boxes.  Start: x = the sphere centres, z = A x, u = 0.  One iteration, fp64, alpha = 1.6:
 *     x = argmin 1/2 x^T Q x + rho/2 |A x - z + u|^2  s.t. E x = b     (H = Q + rho A^T A is block diagonal, one (n+1)x(n+1) block
 *         per segment, the same for x, y and z; w = H^-1 rho A^T (z - u), S nu = E w - b with S = E H^-1 E^T, x = w - H^-1 E^T nu)
 *     v = alpha A x + (1 - alpha) z + u,   z = projection of v onto C,   u = v - z
 * The projection of a control point onto its ball uses radius r - margin - 2 eps.  Every check_every iterations, and at max_iter:
 *     r_prim = max |A x - z|,   r_dual = rho * max |A^T (z - z_before)|      (both in metres: max|Q| = 1)
 * and the stopping test is r_prim <= eps and r_dual <= eps.  The rho rule (params->rho = 0; a positive rho is kept fixed): rho starts
 * at 1e-5; at a check that does not stop,  rho' = rho * sqrt((r_prim / max(|A x|, |z|)) / (r_dual / max(|Q x|, rho |A^T u|))),
 * all norms max-norms, clamped to [1e-9, 1e3]; rho moves to rho' only when they differ by more than a factor 5, and then u is scaled
 * by rho/rho' and H and S are factored again.
 *
 * What PCT_GEN_OK guarantees about the returned numbers.  The final pass recomputes cost, sphere_slack, max_vel_ctrl and
 * max_acc_ctrl from x itself, not from the split variable.  OK requires r_prim <= eps, r_dual <= eps and sphere_slack >= 0, where
 * sphere_slack = the minimum over the control points of (r - margin) - |P - c|: every returned control point is inside its sphere.
 * The shrunk projection radius makes that reachable: when the max-norm residual passes, x is at most sqrt(3) eps < 2 eps from z in
 * the 2-norm.  The returned x satisfies E x = b to roundoff in every status but INVALID.  Velocity and acceleration control values
 * are reported, not guaranteed: they exceed their limit by at most eps * n/T (eps * n(n-1)/T^2) when the status is OK.
 * cost is the objective above in world units, duration the sum of the candidate's seg_time.
 *
 * Output: the wire layout the checks read, polycoef[row][d*(n+1)+j] = P_j[d] / seg_time[row], unused slots of a row written as 0;
 * {d_polycoef, row_stride, seg_time, orders, seg_offsets, NULL, B} is a pct_bezier_batch.
 *
 * Invalid candidates: a non-finite input, seg_time <= 0, radius - margin - 2 eps <= 0, an order outside 5..12 or below
 * minimize_order + 2, fewer than 1 or more than 16 segments.  Each gives PCT_GEN_INVALID for that candidate only: its rows are
 * written as NaN (the whole row_stride), its record holds NaN, the other candidates are untouched.  Bad params -- minimize_order
 * outside 1..4, max_iter <= 0, check_every <= 0, eps not > 0, a NaN limit, margin or rho, rho < 0, a null pointer, B < 0, descending
 * seg_offsets or row_stride < 3 * (max order + 1) in the host form, row_stride < 18 in the device form (it cannot read the orders: there
 * a candidate whose rows do not fit row_stride is INVALID) -- give PCT_ERR_INVALID with nothing written.  An infeasible
 * corridor (disjoint spheres, a start point outside its sphere) gives PCT_GEN_NOT_CONVERGED with the last iterate and honest
 * residuals; it is never OK.  B == 0: PCT_OK.  The device form is asynchronous on `stream`, has no host synchronisation inside and
 * can be captured; the host form copies, calls it and waits once.  A candidate's result does not depend on the rest of the batch:
 * alone or among others it gives the same bytes.
 */
#ifndef PCT_TRAJGEN_H
#define PCT_TRAJGEN_H

#include <stdint.h>

#include "pct_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pct_trajgen_batch {      /* host pointers in the host form, device pointers in the _dev form */
    const double  *centres;      /* total_seg x 3 */
    const double  *radius;       /* total_seg */
    const double  *seg_time;     /* total_seg, > 0 */
    const int32_t *orders;       /* total_seg, each 5..12 */
    const int32_t *seg_offsets;  /* B + 1, as pct_bezier_batch; 1..16 segments per candidate */
    const double  *start_state;  /* B x 9: p, v, a */
    const double  *end_state;    /* B x 9 */
    int64_t        B;
} pct_trajgen_batch;

typedef struct pct_trajgen_params {
    int32_t minimize_order;      /* 1..4 (3 = jerk, the reference's default), <= every order - 2 */
    int32_t max_iter, check_every;
    double  max_vel, max_acc;    /* <= 0 or +inf: no limit */
    double  margin;              /* taken off every radius */
    double  eps;                 /* residual tolerance, metres on the ball rows */
    double  rho;                 /* 0 = automatic */
} pct_trajgen_params;

enum pct_gen_status {
    PCT_GEN_OK = 0,              /* converged, every control point inside its sphere */
    PCT_GEN_NOT_CONVERGED = 1,   /* max_iter reached: the last iterate, honest residuals */
    PCT_GEN_INVALID = 2          /* the candidate's input is unusable: NaN rows */
};

typedef struct pct_trajgen_result {     /* 64 bytes */
    int32_t status;              /* PCT_GEN_OK = 0, PCT_GEN_NOT_CONVERGED = 1, PCT_GEN_INVALID = 2 */
    int32_t iterations;
    double  cost, duration, r_prim, r_dual, sphere_slack, max_vel_ctrl, max_acc_ctrl;
} pct_trajgen_result;

int pct_bezier_generate_batch(const pct_trajgen_batch *batch, const pct_trajgen_params *params, double *polycoef, int64_t row_stride,
                              pct_trajgen_result *result);
int pct_bezier_generate_batch_dev(const pct_trajgen_batch *d_fields, const pct_trajgen_params *params, double *d_polycoef, int64_t row_stride,
                                  pct_trajgen_result *d_res, void *stream);
/* timeAllocation (sim_planning_demo.cpp:603-686) on the host: n spheres -> n segment times.  The joints are the points between
 * neighbouring spheres where their surfaces are equally far; each leg start -> joints -> end gets the time of a trapezoidal speed
 * profile (speed up at acc_mean to vel_mean, cruise, slow down to rest), the first leg starting at init_vel projected on the leg.
 * The reference's statements in the reference's order, fp64.  n < 1, a null pointer, vel_mean or acc_mean not > 0: PCT_ERR_INVALID. */
int pct_time_allocation(const double *centres, const double *radius, int64_t n, const double start[3], const double end[3],
                        const double init_vel[3], double vel_mean, double acc_mean, double *seg_time);

#ifdef __cplusplus
}
#endif
#endif
