// The rectangular linear sum assignment behind pm_assign (include/pasco_match.h): plain C++, no device, no allocation beyond
// std::vector.  Shortest augmenting paths with row and column potentials (the Hungarian method in its O(n^2 m) form): the
// smaller side of the matrix is the side that is augmented, one of its lines per step, so every line of the smaller side ends
// up matched and the total is minimal.  tools/pm_assign_check.cpp holds it to brute force.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace pm_lsa {

// cost [q, t] row-major -> row[k], col[k] for k < min(q, t), rows ascending.  Returns 0, or 1 for a non-finite cost (nothing
// is written then).
inline int solve(const double *cost, int q, int t, int32_t *row, int32_t *col) {
  if (q <= 0 || t <= 0) return 0;
  for (int64_t i = 0; i < (int64_t)q * t; ++i)
    if (!std::isfinite(cost[i])) return 1;
  // augment over the smaller side: lines i = 1..n of it, against the m >= n lines j of the other side
  const bool tr = q > t;
  const int n = tr ? t : q, m = tr ? q : t;
  auto c = [&](int i, int j) { return tr ? cost[(int64_t)j * t + i] : cost[(int64_t)i * t + j]; };
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> u(n + 1, 0.0), v(m + 1, 0.0), minv(m + 1);
  std::vector<int> p(m + 1, 0), way(m + 1, 0);          // p[j] = the line i matched to j (1-based, 0 = free)
  std::vector<char> used(m + 1);
  for (int i = 1; i <= n; ++i) {
    p[0] = i;
    int j0 = 0;
    std::fill(minv.begin(), minv.end(), inf);
    std::fill(used.begin(), used.end(), 0);
    do {
      used[j0] = 1;
      const int i0 = p[j0];
      double delta = inf;
      int j1 = 0;
      for (int j = 1; j <= m; ++j) {
        if (used[j]) continue;
        const double cur = c(i0 - 1, j - 1) - u[i0] - v[j];
        if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
        if (minv[j] < delta) { delta = minv[j]; j1 = j; }
      }
      for (int j = 0; j <= m; ++j) {
        if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
        else minv[j] -= delta;
      }
      j0 = j1;
    } while (p[j0] != 0);
    do {
      const int j1 = way[j0];
      p[j0] = p[j1];
      j0 = j1;
    } while (j0 != 0);
  }
  if (tr) {           // p[j]: j = a row of cost, p[j] = its column; j ascending is already rows ascending
    int k = 0;
    for (int j = 1; j <= m; ++j)
      if (p[j] != 0) { row[k] = j - 1; col[k] = p[j] - 1; ++k; }
  } else {            // p[j]: j = a column, p[j] = its row; order by row
    std::vector<int> col_of(n, -1);
    for (int j = 1; j <= m; ++j)
      if (p[j] != 0) col_of[p[j] - 1] = j - 1;
    for (int i = 0; i < n; ++i) { row[i] = i; col[i] = col_of[i]; }
  }
  return 0;
}

}  // namespace pm_lsa
