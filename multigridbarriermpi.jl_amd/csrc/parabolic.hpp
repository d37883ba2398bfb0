// Step transition of the implicit-Euler time loop of parabolic_solve on gfx950: everything that happens
// to the device state between two barrier solves, so that the loop never takes z to the host.
// Layout: S = 3 state variables [u; s1; s2] column-major in z (3 n), K = dim + 3 rows of D = (u, grad u, s1, s2) row-major in Dz0 / c.
// From t_k to t_{k+1} = t_k + h, in stream order:
//   cost        c[i, 0] = f[i] - u[i] / h (a division, then a subtraction: bitwise numpy's `f - u / h`), c[i, K-2] = 1 / (2h),
//               c[i, K-1] = 1 / p, zero elsewhere;
//   boundary    u[bidx[j]] = gb[j] (a launch of its own BEHIND the cost, which reads the old boundary values);
//   violations  after Dz0 = D z:  v1 = max_i (u_i^2 - s1_i),  v2 = max_i ((sum_d g_id^2)^(p/2) - s2_i),  g = columns 1..dim of Dz0;
//               a node with a non-finite u, g, s1 or s2 contributes NaN and a NaN, once seen, stays (reduce.hpp: nanmax);
//   lifts       lift_j = 1 + v_j if v_j >= 0, exactly 0 if v_j < 0, NaN if v_j is NaN;  s_j += lift_j at every node (a constant
//               shift: the slacks stay in the `full` space); a column whose lift is 0 is not written at all;
//   snapshot    out[i * S + s] = z[s * n + i] (row-major n x S).
// The maxima are reduced by the two-stage scheme of reduce.hpp: one partial pair per workgroup, then ONE workgroup that combines
// the partials in ascending order and computes the lifts.
#pragma once
#include "reduce.hpp"

namespace mgb {
namespace parabolic {

using namespace reduce;          // kThreads, workgroups, nanmax
constexpr int kResults = 4;      // v1, v2, lift_1, lift_2
// one (v1, v2) pair per workgroup, then the kResults results
inline size_t scratch_doubles(int n) { return (size_t)workgroups(n) * 2 + kResults; }
inline size_t results_offset(int n) { return (size_t)workgroups(n) * 2; }

#if defined(__HIPCC__)
// all pointers are device pointers; every launch goes to `stream` and none waits for the host
void launch_cost(hipStream_t stream, int n, int K, double h, double c_s1, double c_s2, const double* f, const double* z, double* c);
void launch_boundary(hipStream_t stream, int nb, const int* bidx, const double* gb, double* z);
// scratch: scratch_doubles(n) doubles; the results land at scratch + results_offset(n)
void launch_violations(hipStream_t stream, int n, int K, double p, const double* z, const double* Dz0, double* scratch);
void launch_lift(hipStream_t stream, int n, const double* lifts2, double* z);
void launch_snapshot(hipStream_t stream, int n, int S, const double* z, double* out);
#endif

}  // namespace parabolic
}  // namespace mgb
