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
 *
 * Trajectory generation in polyhedra (pct_bezier_generate_poly_batch*): the contract.
 *
 * The same problem with another set for the control points: segment g owns the planes [plane_offsets[g], plane_offsets[g+1]), at
 * most pct_trajgen_max_planes() = 24 of them, and every control point of segment g lies in C_g = { y : nh_k . y <= o_k }.  This is
 * what pct_segment_polyhedron_batch produces around a route edge.  The objective, the rows of E, the Gv and Ga boxes, the ADMM
 * iteration, alpha, the residuals, the stopping test, the rho rule, the output layout, B == 0 and the rule that a candidate's bytes
 * do not depend on the rest of the batch are the sphere contract's, word for word; there are no balls in this form (a caller who
 * wants spheres uses pct_bezier_generate_batch).  The planes are normalised once at load: len = |n| = sqrt((n0 n0 + n1 n1) + n2 n2),
 * nh = n / len, o = off / len - margin.  A segment without planes is unconstrained in position: its projection is the identity.
 * Start: x = the segment's anchor for every one of its control points, z = A x, u = 0.
 *
 * The projection.  z = the Euclidean projection of v onto C_g shrunk by 2 eps, { y : g_k(y) <= 0 }, g_k(y) = nh_k . y - (o_k - 2 eps)
 * with nh . y = (nh0 y0 + nh1 y1) + nh2 y2 -- the sphere form's argument: when the max-norm residual passes, x is less than 2 eps from
 * z in the 2-norm.  The point is unique; the algorithm that finds it is pinned, in this order:
 *   1. v itself, if g_k(v) <= 0 for every k (no tolerance: then u = 0 exactly).
 *   2. The KKT enumeration over active sets of one plane (i ascending), then two (i < j, i outer), then three (i < j < k).  The
 *      candidate is the point on those planes nearest v, y = v - sum l_q nh_q, its multipliers l solving the Gram system of the unit
 *      normals in closed form: l_i = g_i(v); with a = nh_i . nh_j, det = 1 - a a, l_i = (g_i - a g_j) / det, l_j = (g_j - a g_i) / det;
 *      with b = nh_i . nh_k, c = nh_j . nh_k, det = ((1 + 2 ((a b) c)) - (a a + b b)) - c c and l = adj(G) g / det.  A pair or triple
 *      with det < 1e-8 is skipped as near-parallel (a triple also when its first pair is).  A candidate counts when every multiplier
 *      is >= 0; its worst violation w is the largest g_q(y) over the planes outside its active set (-inf when there are none).  The
 *      first candidate with w <= 1e-9 (the accept tolerance, metres) is z.
 *   3. Where rounding lets no active set pass -- or the set is empty -- z is the counting candidate with the smallest w, kept as
 *      the enumeration goes: the first counting candidate is kept, and a later one takes its place only when its w is better by more
 *      than 1e-9, so that rounding does not decide between equals.  There always is one: a plane v violates is a counting active
 *      set of one.  The point is not moved further: the status below does not trust it.
 * The two constants against the coordinates' ulp: a world of |y| <= 1e3 m has ulp <= 1.2e-13 m, so g carries an error of a few
 * 1e-13; a Gram system with det >= 1e-8 (planes at an angle >= 1e-4 rad) magnifies that by at most about 1 / sqrt(det) = 1e4 in the
 * candidate, to about 1e-9, the accept tolerance; and 1e-9 is four orders below the eps the solver is run at.  The previous
 * iteration's active set is not tried first: the form kept is the plain enumeration.
 *
 * Results.  sphere_slack is, for this call, the corridor slack: the minimum over the control points and their planes of
 * o_k - nh_k . P, the margin taken off and no 2 eps, recomputed from the returned x in the final pass (+inf for a candidate without
 * planes).  PCT_GEN_OK requires r_prim <= eps, r_dual <= eps and slack >= 0: OK means every returned control point is inside every
 * plane moved in by the margin, whatever the projection did -- the status does not lean on the two constants above -- and, a Bezier
 * segment lying in the hull of its control points, the whole curve is in the polytope.
 *
 * Invalid candidates (PCT_GEN_INVALID, NaN rows, the other candidates untouched): the sphere form's conditions without the radius
 * one, and a non-finite anchor; a non-finite plane or a plane whose |n| as computed above is 0 or not finite; more than 24 planes on
 * one segment; plane_offsets descending inside the candidate.  An infeasible chain -- an empty polytope, a start point outside its
 * polytope, two neighbouring polytopes without a common point -- ends as PCT_GEN_NOT_CONVERGED with honest residuals, never OK.  The
 * host form gives PCT_ERR_INVALID with nothing written for a null pointer, plane_offsets[0] != 0 or a descent of plane_offsets
 * anywhere, besides the sphere form's reasons; the device form cannot read the offsets and leaves them to the candidates.
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
typedef struct pct_trajgen_poly_batch {   /* host pointers in the host form, device pointers in the _dev form */
    const double  *anchors;        /* total_seg x 3: the start iterate of the segment's control points (e.g. the edge midpoint) */
    const double  *planes;         /* total_planes x 4: n0 n1 n2 off, the half-space n . y <= off; n need not be a unit vector */
    const int32_t *plane_offsets;  /* total_seg + 1, ascending, plane_offsets[0] = 0: segment g owns planes [po[g], po[g+1]) */
    const double  *seg_time;       /* total_seg, > 0 */
    const int32_t *orders;         /* total_seg, each 5..12 */
    const int32_t *seg_offsets;    /* B + 1 */
    const double  *start_state;    /* B x 9: p, v, a */
    const double  *end_state;      /* B x 9 */
    int64_t        B;
} pct_trajgen_poly_batch;

/* The polyhedral corridor ("Trajectory generation in polyhedra" above); sphere_slack of the record is the corridor slack. */
int pct_bezier_generate_poly_batch(const pct_trajgen_poly_batch *batch, const pct_trajgen_params *params, double *polycoef, int64_t row_stride,
                                   pct_trajgen_result *result);
int pct_bezier_generate_poly_batch_dev(const pct_trajgen_poly_batch *d_fields, const pct_trajgen_params *params, double *d_polycoef, int64_t row_stride,
                                       pct_trajgen_result *d_res, void *stream);
int pct_trajgen_max_planes(void);         /* 24: the most planes one segment may own */

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
