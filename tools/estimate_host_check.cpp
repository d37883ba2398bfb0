// Stand-alone check of the host code behind the error indicators: boundary::build_facet_lists (interior
// facets, element -> facet table) and the host restatement estimate::estimate_host, over fem1d, fem2d with and without K, a
// single triangle, fem3d k = 1..3 at L <= 3 (k = 3: L <= 2), with and without forcing, Neumann data and a mask, r = 1, 2, 1.5,
// both scales, and the refused mesh whose sides do not match.  Meant to be built with a sanitizer and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I multigridbarriermpi.jl_amd/csrc \
//       tools/estimate_host_check.cpp multigridbarriermpi.jl_amd/csrc/geometry.cpp -o tools/_bin/estimate_host_check
// Exit status 0 and "estimate_host_check ok" when every property holds.
#include <cstdio>
#include <cstdlib>

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

template <class F>
static bool refused(F&& fn) {
  try {
    fn();
  } catch (const ArgError&) {
    return true;
  }
  return false;
}

static void check_geometry(const char* name, const GeometryHost& g) {
  boundary::Facets F;
  boundary::Interior I;
  boundary::build_facet_lists(g, &F, &I);
  const boundary::Facets F0 = boundary::build_facets(g);
  CHECK(F0.nodes == F.nodes && F0.weights == F.weights && F0.normal == F.normal && F0.element == F.element);
  const int q = I.q, dim = I.dim, block = g.block;
  CHECK(I.nel * block == g.n && I.nel * I.nlf == 2 * I.nif + F.nf);
  std::vector<int> seen_i((size_t)I.nif, 0), seen_b((size_t)F.nf, 0);
  for (int t : I.elem_facet) {
    CHECK(t >= -F.nf && t < I.nif);
    if (t >= 0) seen_i[t]++;
    else seen_b[-1 - t]++;
  }
  for (int v : seen_i) CHECK(v == 2);
  for (int v : seen_b) CHECK(v == 1);
  for (int f = 0; f < I.nif; ++f) {
    CHECK(I.elements[2 * f] < I.elements[2 * f + 1]);
    double nn = 0.0, ws = 0.0;
    for (int d = 0; d < dim; ++d) nn += I.normal[(size_t)f * dim + d] * I.normal[(size_t)f * dim + d];
    CHECK(std::fabs(nn - 1.0) <= 1e-14);
    for (int j = 0; j < q; ++j) {
      const int a = I.nodes[((size_t)f * 2) * q + j], b = I.nodes[((size_t)f * 2 + 1) * q + j];
      CHECK(a / block == I.elements[2 * f] && b / block == I.elements[2 * f + 1]);
      for (int d = 0; d < dim; ++d) CHECK(g.x[(size_t)a * dim + d] == g.x[(size_t)b * dim + d]);
      ws += I.weights[(size_t)f * q + j];
    }
    CHECK(std::fabs(ws - I.measure[f]) <= 1e-14 * I.measure[f]);
  }
  // the indicator on a broken field: finite and non-negative, a masked-out NaN not read, repeatable
  const int n = g.n, S = 2;
  std::vector<double> z((size_t)n * S), f((size_t)n), h((size_t)F.nf * q), sigma((size_t)n * dim);
  unsigned s = 12345u;
  auto rnd = [&] {
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / 8388608.0 - 1.0;
  };
  for (double& v : z) v = rnd();
  for (double& v : f) v = rnd();
  for (double& v : h) v = rnd();
  std::vector<unsigned char> mask((size_t)F.nf);
  for (int t = 0; t < F.nf; ++t) mask[t] = t % 3 != 1;
  for (double p : {1.0, 1.5, 2.0, 3.0})
    for (double r : {1.0, 2.0, 1.5})
      for (int own_scale = 0; own_scale < 2; ++own_scale)
        for (int neu = 0; neu < 2; ++neu) {
          energy::Args E;
          E.own.block = block, E.own.nel = I.nel, E.own.x = g.x.data();
          E.w = g.w.data(), E.p = p;
          E.n = n, E.S = S, E.u = 0, E.B = 1;
          estimate::field_flux_host(dim, F.k, E, z.data(), sigma.data());
          estimate::Args A;
          A.own = E.own;
          A.w = E.w, A.p = p, A.sigma = sigma.data(), A.f = neu ? f.data() : nullptr;
          A.r = r, A.scale = 0.75, A.own_scale = own_scale != 0;
          A.n = n, A.nel = I.nel, A.nlf = I.nlf, A.q = q;
          A.inodes = I.nodes.data(), A.iweights = I.weights.data(), A.inormal = I.normal.data(), A.nif = I.nif;
          A.bnodes = F.nodes.data(), A.bweights = F.weights.data(), A.bnormal = F.normal.data(), A.nf = F.nf;
          A.mask = neu ? mask.data() : nullptr, A.h = neu ? h.data() : nullptr;
          A.elem_facet = I.elem_facet.data();
          std::vector<double> eta((size_t)I.nel * 3, -1.0), J((size_t)I.nif, -1.0), N((size_t)F.nf, -1.0), eta2(eta), J2(J), N2(N);
          double out[5], out2[5];
          estimate::estimate_host(dim, F.k, A, eta.data(), J.data(), N.data(), out);
          for (double v : eta) CHECK(v >= 0.0 && std::isfinite(v));
          for (double v : J) CHECK(v >= 0.0 && std::isfinite(v));
          for (int k = 0; k < 5; ++k) CHECK(out[k] >= 0.0 && std::isfinite(out[k]));
          if (neu) {
            for (int t = 0; t < F.nf; ++t) CHECK(mask[t] ? N[t] >= 0.0 : N[t] == 0.0);
            std::vector<double> hn(h);
            for (int t = 0; t < F.nf; ++t)
              if (!mask[t])
                for (int j = 0; j < q; ++j) hn[(size_t)t * q + j] = std::numeric_limits<double>::quiet_NaN();
            A.h = hn.data();
            estimate::estimate_host(dim, F.k, A, eta2.data(), J2.data(), N2.data(), out2);
            CHECK(eta == eta2 && J == J2 && N == N2);
            for (int k = 0; k < 5; ++k) CHECK(out[k] == out2[k]);
          } else {
            CHECK(out[2] == 0.0);
          }
        }
  std::printf("%-16s n %6d  L %d  interior facets %5d x %2d  boundary facets %5d\n", name, g.n, g.L, I.nif, q, F.nf);
}

int main() {
  const double Lshape[] = {-1, -1, 0, -1, 0, 0, -1, -1, 0, 0, -1, 0, 0, -1, 1, -1, 1, 0, 0, -1, 1, 0, 0, 0, -1, 0, 0, 0, 0, 1, -1, 0, 0, 1, -1, 1};
  for (int L = 1; L <= 3; ++L) {
    char name[64];
    std::snprintf(name, sizeof name, "fem1d L=%d", L);
    check_geometry(name, fem1d_native(L));
    std::snprintf(name, sizeof name, "fem2d L=%d", L);
    check_geometry(name, fem2d_native(L, nullptr, 0));
    std::snprintf(name, sizeof name, "fem2d K L=%d", L);
    check_geometry(name, fem2d_native(L, Lshape, 18));
    std::snprintf(name, sizeof name, "triangle L=%d", L);
    check_geometry(name, fem2d_native(L, Lshape, 3));
    for (int k = 1; k <= 3; ++k) {
      if (k == 3 && L == 3) continue;
      std::snprintf(name, sizeof name, "fem3d k=%d L=%d", k, L);
      check_geometry(name, fem3d_native(L, k));
    }
  }
  // refused: the midpoint of one side of an interior edge on a dof of its own; no full subspace
  GeometryHost g = fem2d_native(2, nullptr, 0);
  const boundary::Interior I = boundary::build_interior(g);
  GeometryHost bad = g;
  Csr& full = bad.subspaces["full"][bad.L - 1];
  full.colidx[full.rowptr[I.nodes[(size_t)I.q + 1]]] = full.cols;
  full.cols += 1;
  CHECK(refused([&] { boundary::build_interior(bad); }));
  GeometryHost no_full = g;
  no_full.subspaces.erase("full");
  CHECK(refused([&] { boundary::build_interior(no_full); }));
  if (failures) {
    std::fprintf(stderr, "estimate_host_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("estimate_host_check ok\n");
  return 0;
}
