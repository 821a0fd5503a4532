// Stand-alone check of the assignment solver behind pm_assign (pasco_amd/csrc/pm_assign.h): no GPU, no library, its own main.
// Build it with the host compiler and the sanitizers, e.g.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/pm_assign_check.cpp -o pm_assign_check && ./pm_assign_check
//
// 1. Every Q, T <= 5, three seeded matrices each (plain, ties = integers 0..2, equal columns): the total equals brute force over
//    all injections of the smaller side, and the result has the documented form (K = min(Q, T) pairs, rows ascending, no row or
//    column twice).  tests/match_cases.py builds the same matrices from the same generator and runs them through the library.
// 2. Seeded 100 x 30, 30 x 100 and 128 x 128 matrices: a valid assignment that no exchange improves - swapping the partners of
//    any two matched pairs, or moving a pair to an unmatched row or an unmatched column.
// 3. A non-finite cost is refused and writes nothing.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../pasco_amd/csrc/pm_assign.h"

namespace {

struct Lcg {                     // the generator tests/match_cases.py restates
  uint64_t s;
  explicit Lcg(uint64_t seed) : s(seed) {}
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  }
};

std::vector<double> make_cost(int q, int t, int kind) {
  Lcg g(17ull * q + t + 1000ull * kind);
  std::vector<double> c((size_t)q * t);
  for (double &v : c) v = g.next();
  if (kind == 1)
    for (double &v : c) v = (double)(int)(v * 3.0);
  if (kind == 2)
    for (int i = 0; i < q; ++i)
      for (int j = 1; j < t; ++j) c[(size_t)i * t + j] = c[(size_t)i * t];
  return c;
}

int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      std::printf("FAIL: ");        \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
    }                               \
  } while (0)

bool well_formed(int q, int t, const std::vector<int32_t> &row, const std::vector<int32_t> &col) {
  const int k = std::min(q, t);
  std::vector<char> ur(q, 0), uc(t, 0);
  for (int i = 0; i < k; ++i) {
    if (row[i] < 0 || row[i] >= q || col[i] < 0 || col[i] >= t) return false;
    if (i > 0 && row[i] <= row[i - 1]) return false;
    if (ur[row[i]] || uc[col[i]]) return false;
    ur[row[i]] = uc[col[i]] = 1;
  }
  return true;
}

double total(const std::vector<double> &c, int t, const std::vector<int32_t> &row, const std::vector<int32_t> &col) {
  double s = 0.0;
  for (size_t i = 0; i < row.size(); ++i) s += c[(size_t)row[i] * t + col[i]];
  return s;
}

// the minimum over all injections of the smaller side into the larger
double brute(const std::vector<double> &c, int q, int t) {
  const bool tr = q > t;
  const int n = tr ? t : q, m = tr ? q : t;
  std::vector<int> perm(m);
  for (int j = 0; j < m; ++j) perm[j] = j;
  double best = std::numeric_limits<double>::infinity();
  do {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += tr ? c[(size_t)perm[i] * t + i] : c[(size_t)i * t + perm[i]];
    best = std::min(best, s);
  } while (std::next_permutation(perm.begin(), perm.end()));
  return best;
}

void check_small() {
  for (int q = 1; q <= 5; ++q)
    for (int t = 1; t <= 5; ++t)
      for (int kind = 0; kind < 3; ++kind) {
        const std::vector<double> c = make_cost(q, t, kind);
        const int k = std::min(q, t);
        std::vector<int32_t> row(k, -7), col(k, -7);
        CHECK(pm_lsa::solve(c.data(), q, t, row.data(), col.data()) == 0, "%d x %d kind %d refused", q, t, kind);
        CHECK(well_formed(q, t, row, col), "%d x %d kind %d: malformed result", q, t, kind);
        const double got = total(c, t, row, col), want = brute(c, q, t);
        CHECK(got - want <= 1e-12 && want - got <= 1e-12, "%d x %d kind %d: total %.17g, brute force %.17g", q, t, kind, got, want);
      }
}

void check_exchange(int q, int t, uint64_t seed) {
  Lcg g(seed);
  std::vector<double> c((size_t)q * t);
  for (double &v : c) v = g.next() * 4.0 - 2.0;
  const int k = std::min(q, t);
  std::vector<int32_t> row(k, -7), col(k, -7);
  CHECK(pm_lsa::solve(c.data(), q, t, row.data(), col.data()) == 0, "%d x %d refused", q, t);
  CHECK(well_formed(q, t, row, col), "%d x %d: malformed result", q, t);
  if (!well_formed(q, t, row, col)) return;
  auto at = [&](int i, int j) { return c[(size_t)i * t + j]; };
  const double eps = 1e-12;
  for (int a = 0; a < k; ++a)
    for (int b = a + 1; b < k; ++b)
      CHECK(at(row[a], col[b]) + at(row[b], col[a]) >= at(row[a], col[a]) + at(row[b], col[b]) - eps,
            "%d x %d: swapping pairs %d and %d improves", q, t, a, b);
  std::vector<char> ur(q, 0), uc(t, 0);
  for (int i = 0; i < k; ++i) ur[row[i]] = uc[col[i]] = 1;
  for (int a = 0; a < k; ++a) {
    for (int i = 0; i < q; ++i)
      if (!ur[i]) CHECK(at(i, col[a]) >= at(row[a], col[a]) - eps, "%d x %d: unmatched row %d improves pair %d", q, t, i, a);
    for (int j = 0; j < t; ++j)
      if (!uc[j]) CHECK(at(row[a], j) >= at(row[a], col[a]) - eps, "%d x %d: unmatched column %d improves pair %d", q, t, j, a);
  }
}

void check_refusal() {
  std::vector<double> c = make_cost(4, 3, 0);
  std::vector<int32_t> row(3, -7), col(3, -7);
  c[7] = std::numeric_limits<double>::quiet_NaN();
  CHECK(pm_lsa::solve(c.data(), 4, 3, row.data(), col.data()) == 1, "NaN accepted");
  c[7] = std::numeric_limits<double>::infinity();
  CHECK(pm_lsa::solve(c.data(), 4, 3, row.data(), col.data()) == 1, "inf accepted");
  for (int i = 0; i < 3; ++i) CHECK(row[i] == -7 && col[i] == -7, "a refused call wrote its outputs");
  CHECK(pm_lsa::solve(nullptr, 0, 3, nullptr, nullptr) == 0 && pm_lsa::solve(nullptr, 3, 0, nullptr, nullptr) == 0, "empty matrix");
}

}  // namespace

int main() {
  check_small();
  check_exchange(100, 30, 1);
  check_exchange(30, 100, 2);
  check_exchange(128, 128, 3);
  check_refusal();
  if (failures != 0) {
    std::printf("pm_assign_check: %d failures\n", failures);
    return 1;
  }
  std::printf("pm_assign_check: ok\n");
  return 0;
}
