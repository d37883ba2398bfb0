// Stand-alone check of the host restatement of the error indicators of parabolic steps:
// estimate::estimate_host with Args::steps over fem1d L=2, fem2d L=2 and fem3d L=1 k=3, B = 3 unequal steps, four exponents, three
// powers, with and without forcing (one row and B rows), Neumann data (one row and B rows) and a mask.  Properties: every number
// finite and non-negative, a batch equal to its steps one by one, a repeated snapshot giving the single field's numbers and a
// zero time part, a NaN in snapshot 1 reaching steps 1 and 2 only.  Meant to be built with a sanitizer and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I multigridbarriermpi.jl_amd/csrc \
//       tools/estimate_steps_host_check.cpp multigridbarriermpi.jl_amd/csrc/geometry.cpp -o tools/_bin/estimate_steps_host_check
// Exit status 0 and "estimate_steps_host_check ok" when every property holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "estimate.hpp"

using namespace mgb;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

struct Run {
  std::vector<double> sigma, parts, J, N, out;
};

static bool same_bits(const double* a, const double* b, size_t count) {
  return count == 0 || std::memcmp(a, b, count * sizeof(double)) == 0;      // no interior facet: nothing to compare, null pointers
}

// the steps first .. first + B - 1 of the snapshots zs at the times ts
static Run run(const GeometryHost& g, const boundary::Facets& F, const boundary::Interior& I, const std::vector<const double*>& zs,
               const std::vector<double>& ts, int first, int B, int S, double p, double r, const double* f, int f_rows, const double* h,
               int h_rows, const unsigned char* mask, bool steps = true) {
  const int n = g.n, dim = I.dim;
  const size_t nsig = (size_t)n * dim;
  Run R;
  R.sigma.assign((size_t)(B + 1) * nsig, -1.0);
  energy::Args E;
  E.own.block = g.block, E.own.nel = I.nel, E.own.x = g.x.data();
  E.w = g.w.data(), E.p = p;
  E.n = n, E.S = S, E.u = 0, E.B = 1;
  for (int b = 0; b <= (steps ? B : 0); ++b) estimate::field_flux_host(dim, F.k, E, zs[first + b], R.sigma.data() + (size_t)b * nsig);
  std::vector<double> dt((size_t)B);
  for (int k = 0; k < B; ++k) dt[k] = ts[first + k + 1] - ts[first + k];
  estimate::Args A;
  A.own = E.own;
  A.w = E.w, A.p = p, A.sigma = R.sigma.data(), A.f = f;
  A.r = r, A.scale = 0.75, A.own_scale = true;
  A.n = n, A.nel = I.nel, A.nlf = I.nlf, A.q = I.q;
  A.inodes = I.nodes.data(), A.iweights = I.weights.data(), A.inormal = I.normal.data(), A.nif = I.nif;
  A.bnodes = F.nodes.data(), A.bweights = F.weights.data(), A.bnormal = F.normal.data(), A.nf = F.nf;
  A.mask = h ? mask : nullptr, A.h = h;
  A.elem_facet = I.elem_facet.data();
  if (steps) {
    A.B = B, A.steps = true;
    A.z = zs.data() + first, A.S = S, A.u = 0, A.dt = dt.data();
    A.f_stride = f && f_rows == B && B > 1 ? n : 0;
    A.h_stride = h && h_rows == B && B > 1 ? (long long)F.nf * I.q : 0;
  }
  R.parts.assign((size_t)B * I.nel * estimate::parts_of(A), -1.0);
  R.J.assign((size_t)B * I.nif, -1.0);
  R.N.assign((size_t)B * F.nf, -1.0);
  R.out.assign((size_t)B * estimate::rows_of(A) * 5, -1.0);
  estimate::estimate_host(dim, F.k, A, R.parts.data(), R.J.data(), R.N.data(), R.out.data());
  return R;
}

static void check_geometry(const char* name, const GeometryHost& g) {
  boundary::Facets F;
  boundary::Interior I;
  boundary::build_facet_lists(g, &F, &I);
  const int n = g.n, S = 2, B = 3, q = I.q, nel = I.nel;
  const std::vector<double> ts = {0.0, 0.3, 0.5, 1.0};
  unsigned s = 4321u;
  auto rnd = [&] {
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / 8388608.0 - 1.0;
  };
  std::vector<std::vector<double>> z(B + 1, std::vector<double>((size_t)n * S));
  for (auto& zk : z)
    for (double& v : zk) v = rnd();
  std::vector<double> f((size_t)B * n), h((size_t)B * F.nf * q);
  for (double& v : f) v = rnd();
  for (double& v : h) v = rnd();
  std::vector<unsigned char> mask((size_t)F.nf);
  for (int t = 0; t < F.nf; ++t) mask[t] = t % 3 != 1;
  std::vector<const double*> zs;
  for (auto& zk : z) zs.push_back(zk.data());
  const size_t np = (size_t)nel * 4;
  for (double p : {1.0, 1.5, 2.0, 3.0})
    for (double r : {1.0, 2.0, 1.5})
      for (int variant = 0; variant < 4; ++variant) {
        const double* fp = variant == 0 ? nullptr : f.data();
        const int f_rows = variant >= 2 ? B : 1;
        const double* hp = variant == 0 || variant == 3 ? nullptr : h.data();
        const int h_rows = variant == 2 ? B : 1;
        const Run R = run(g, F, I, zs, ts, 0, B, S, p, r, fp, f_rows, hp, h_rows, mask.data());
        for (double v : R.parts) CHECK(v >= 0.0 && std::isfinite(v));
        for (double v : R.out) CHECK(v >= 0.0 && std::isfinite(v));
        for (int b = 0; b < B; ++b) CHECK(R.out[(size_t)b * 10 + 7] == 0.0);
        // a batch is its steps one by one
        for (int b = 0; b < B; ++b) {
          const Run one = run(g, F, I, zs, ts, b, 1, S, p, r, fp ? fp + (f_rows == B ? (size_t)b * n : 0) : nullptr, 1,
                              hp ? hp + (h_rows == B ? (size_t)b * F.nf * q : 0) : nullptr, 1, mask.data());
          CHECK(same_bits(one.parts.data(), R.parts.data() + b * np, np) && same_bits(one.out.data(), R.out.data() + (size_t)b * 10, 10));
          CHECK(same_bits(one.J.data(), R.J.data() + (size_t)b * I.nif, I.nif) && same_bits(one.sigma.data(), R.sigma.data() + (size_t)b * n * I.dim, 2 * (size_t)n * I.dim));
        }
        // snapshots 1 and 2 equal: step 2 is the single field with own_scale, its time part exactly 0
        std::vector<const double*> eq = {zs[0], zs[1], zs[1], zs[3]};
        const Run Q = run(g, F, I, eq, ts, 0, B, S, p, r, fp, f_rows, hp, h_rows, mask.data());
        const Run single = run(g, F, I, eq, ts, 2, 1, S, p, r, fp ? fp + (f_rows == B ? (size_t)n : 0) : nullptr, 1,
                               hp ? hp + (h_rows == B ? (size_t)F.nf * q : 0) : nullptr, 1, mask.data(), false);
        for (int e = 0; e < nel; ++e) {
          CHECK(same_bits(Q.parts.data() + np + (size_t)e * 4, single.parts.data() + (size_t)e * 3, 3));
          CHECK(Q.parts[np + (size_t)e * 4 + 3] == 0.0);
        }
        CHECK(same_bits(Q.out.data() + 10, single.out.data(), 5));
        for (int k = 0; k < 5; ++k) CHECK(Q.out[15 + k] == 0.0);
        // a NaN in snapshot 1 reaches steps 1 and 2 and no other
        std::vector<double> z1(z[1]);
        z1[(size_t)(nel / 2) * g.block * S] = std::numeric_limits<double>::quiet_NaN();
        std::vector<const double*> bad = {zs[0], z1.data(), zs[2], zs[3]};
        const Run W = run(g, F, I, bad, ts, 0, B, S, p, r, fp, f_rows, hp, h_rows, mask.data());
        CHECK(std::isnan(W.out[0]) && std::isnan(W.out[5]) && std::isnan(W.out[10]) && std::isnan(W.out[15]) && std::isnan(W.out[19]));
        CHECK(same_bits(W.parts.data() + 2 * np, R.parts.data() + 2 * np, np) && same_bits(W.out.data() + 20, R.out.data() + 20, 10));
      }
  std::printf("%-16s n %6d  interior facets %5d x %2d  boundary facets %5d\n", name, g.n, I.nif, q, F.nf);
}

int main() {
  check_geometry("fem1d L=2", fem1d_native(2));
  check_geometry("fem2d L=2", fem2d_native(2, nullptr, 0));
  check_geometry("fem3d k=3 L=1", fem3d_native(1, 3));
  if (failures) {
    std::fprintf(stderr, "estimate_steps_host_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("estimate_steps_host_check ok\n");
  return 0;
}
