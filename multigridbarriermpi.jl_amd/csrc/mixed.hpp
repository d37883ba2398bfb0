// Dirichlet conditions on part of the boundary: a subspace family "sub:<name>:<l>" of a geometry that
// pins u on the rows of the selected boundary facets and leaves the rest of the boundary free.  Host only, built once.
//   The pinned rows are the rows of the selected facets of boundary::build_facets; the set is closed, the end points of a
//   selected facet belong to it.
//   Column rule, per level l, applied to sub:full:<l> (n x m_l, rows of the FINEST mesh): a column is dropped when it has a
//   non-zero value in a pinned row; stored zeros do not count.  Kept columns keep their order and their bits, stored zeros
//   included.  Because the rule looks at the prolonged column, a coarse function that would move a pinned fine value is removed:
//   the coarse spaces stay inside the fine one.  Every facet selected reproduces "dirichlet", none reproduces "full".
#pragma once
#include <string>

#include "boundary.hpp"

namespace mgb {
namespace mixed {

// one flag per row of the finest mesh: 1 on the rows of the selected facets (mask null: every facet)
inline std::vector<unsigned char> pinned_rows(int n, const boundary::Facets& F, const unsigned char* facet_mask) {
  std::vector<unsigned char> pinned((size_t)n, 0);
  for (int f = 0; f < F.nf; ++f) {
    if (facet_mask && !facet_mask[f]) continue;
    for (int j = 0; j < F.q; ++j) pinned[(size_t)F.nodes[(size_t)f * F.q + j]] = 1;
  }
  return pinned;
}

// the columns of A without those that have a non-zero value in a pinned row
inline Csr drop_pinned_columns(const Csr& A, const std::vector<unsigned char>& pinned) {
  std::vector<int> newcol((size_t)A.cols, 0);      // 0 kept, -1 dropped; then the new index
  for (int r = 0; r < A.rows; ++r) {
    if (!pinned[(size_t)r]) continue;
    for (int e = A.rowptr[r]; e < A.rowptr[r + 1]; ++e)
      if (A.vals[e] != 0.0) newcol[(size_t)A.colidx[e]] = -1;
  }
  int kept = 0;
  for (int c = 0; c < A.cols; ++c)
    if (newcol[(size_t)c] == 0) newcol[(size_t)c] = kept++;
  Csr R(A.rows, kept);
  R.colidx.reserve(A.colidx.size());
  R.vals.reserve(A.vals.size());
  for (int r = 0; r < A.rows; ++r) {
    for (int e = A.rowptr[r]; e < A.rowptr[r + 1]; ++e) {
      const int c = newcol[(size_t)A.colidx[e]];
      if (c < 0) continue;
      R.colidx.push_back(c);      // kept columns keep their order: a sorted row stays sorted
      R.vals.push_back(A.vals[e]);
    }
    R.rowptr[(size_t)r + 1] = (int)R.colidx.size();
  }
  return R;
}

// adds subspaces[name][l] for every level; throws ArgError before anything is added
inline void dirichlet_on(GeometryHost& g, const std::string& name, const unsigned char* facet_mask) {
  if (name.empty() || name.find(':') != std::string::npos) throw ArgError("dirichlet_on: the name must be non-empty and without ':'");
  if (name == "full" || name == "dirichlet" || name == "fixed") throw ArgError("dirichlet_on: the name '" + name + "' is taken");
  if (g.subspaces.count(name)) throw ArgError("dirichlet_on: the geometry already has a subspace '" + name + "'");
  auto it = g.subspaces.find("full");
  if (it == g.subspaces.end()) throw ArgError("dirichlet_on: the geometry has no full subspace");
  if (g.L < 1 || (int)it->second.size() != g.L) throw ArgError("dirichlet_on: a level of the full subspace is missing");
  for (const Csr& A : it->second)
    if (A.rows != g.n || (int)A.rowptr.size() != g.n + 1) throw ArgError("dirichlet_on: a level of the full subspace is missing");
  const boundary::Facets F = boundary::build_facets(g);
  const std::vector<unsigned char> pinned = pinned_rows(g.n, F, facet_mask);
  std::vector<Csr> out;
  out.reserve((size_t)g.L);
  for (const Csr& A : it->second) out.push_back(drop_pinned_columns(A, pinned));
  g.subspaces[name] = std::move(out);
}

}  // namespace mixed
}  // namespace mgb
