// wgrad_plan_check.cpp - host check of the weight gradient's team plan (warpconvnet_amd/csrc/wgrad_plan.h), the very text
// the kernel compiles.  Stand-alone; build it with sanitizers and run it directly:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I warpconvnet_amd/csrc \
//       tools/wgrad_plan_check.cpp -o /tmp/wgrad_plan_check && /tmp/wgrad_plan_check
//
// For every table - 3 x 3 x 3 maps of small random scenes built here the way the kernel-map scan builds them, and
// adversarial hand-made ones - the segments of all 512 workgroups must cover every pair position of [0, L) exactly once, stay
// inside one bucket, and an own range must be exactly its (slab, offset) range.  Where the AUTO rule holds, the step counts of
// the workgroups differ by at most one.  Exit status 0 = all held.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "wgrad_plan.h"

using namespace wcn;

static int g_failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAIL %s:%d  ", __FILE__, __LINE__);    \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      ++g_failures;                                       \
    }                                                     \
  } while (0)

struct Tables {
  std::vector<int32_t> offsets;  // [K + 1]
  std::vector<int32_t> bounds;   // [17][K]
};

// bounds from per-(offset, 256-row tile) pair counts, as kmap_scan_kernel forms them: ntile rounded up to a multiple of 4,
// ceil(ntile / 16) tiles per slab, bounds[t][k] = pairs of bucket k in the tiles in front of slab t
static Tables tables_from_counts(const std::vector<std::vector<int>>& counts, int64_t rows) {
  const int K = (int)counts.size();
  const int64_t ntile = (((rows + 255) / 256) + 3) & ~(int64_t)3;
  const int64_t tps = (ntile + kPlanSlabs - 1) / kPlanSlabs;
  Tables t;
  t.offsets.assign(K + 1, 0);
  t.bounds.assign((size_t)(kPlanSlabs + 1) * K, 0);
  for (int k = 0; k < K; ++k) {
    std::vector<int64_t> scan(ntile + 1, 0);
    for (int64_t i = 0; i < ntile; ++i) scan[i + 1] = scan[i] + (i < (int64_t)counts[k].size() ? counts[k][i] : 0);
    for (int s = 0; s <= kPlanSlabs; ++s) t.bounds[(size_t)s * K + k] = (int32_t)scan[std::min<int64_t>(s * tps, ntile)];
    t.offsets[k + 1] = t.offsets[k] + (int32_t)scan[ntile];
  }
  return t;
}

// n distinct random voxels of a side^3 box in random row order (side^3 <= n: the full cube) -> tile counts of the 27 offsets
static Tables scene_tables(int64_t n, int side, uint32_t seed) {
  std::mt19937 rng(seed);
  std::vector<int32_t> cells((size_t)side * side * side);
  for (size_t i = 0; i < cells.size(); ++i) cells[i] = (int32_t)i;
  std::shuffle(cells.begin(), cells.end(), rng);
  if ((int64_t)cells.size() > n) cells.resize((size_t)n);
  n = (int64_t)cells.size();
  std::unordered_map<int32_t, int32_t> row_of;
  for (int64_t r = 0; r < n; ++r) row_of[cells[r]] = (int32_t)r;
  std::vector<std::vector<int>> counts(27, std::vector<int>((size_t)((n + 255) / 256), 0));
  for (int64_t r = 0; r < n; ++r) {
    const int c = cells[r], x = c / (side * side), y = (c / side) % side, z = c % side;
    for (int k = 0; k < 27; ++k) {
      const int nx = x + k / 9 - 1, ny = y + (k / 3) % 3 - 1, nz = z + k % 3 - 1;
      if (nx < 0 || ny < 0 || nz < 0 || nx >= side || ny >= side || nz >= side) continue;
      if (row_of.count((nx * side + ny) * side + nz)) ++counts[k][(size_t)(r / 256)];
    }
  }
  return tables_from_counts(counts, n);
}

static int64_t check_tables(const char* name, const Tables& t, int mode, bool expect_team) {
  const int K = (int)t.offsets.size() - 1, G = kPlanGrid;
  const int32_t* off = t.offsets.data();
  const int32_t* bd = t.bounds.empty() ? nullptr : t.bounds.data();
  const bool team = wgrad_team_rule_all(off, bd, K, G, 1, mode);
  CHECK(team == expect_team, "%s: rule says %d, expected %d", name, (int)team, (int)expect_team);
  if (!team) return -1;
  const int64_t L = off[K];
  std::vector<uint8_t> seen((size_t)L, 0);
  int64_t smin = INT64_MAX, smax = 0;
  for (int g = 0; g < G; ++g) {
    WgradSeg seg[2];
    const int n = wgrad_team_plan(off, bd, K, G, g, seg);
    int t_, m_;
    const bool member = wgrad_member(g, &t_, &m_);
    CHECK(n == (member ? 2 : 1), "%s: g %d has %d segments", name, g, n);
    int64_t steps = 0;
    for (int s = 0; s < n; ++s) {
      const WgradSeg& q = seg[s];
      CHECK(q.k >= 0 && q.k < K, "%s: g %d bucket %d", name, g, q.k);
      CHECK(q.begin <= q.end && q.begin >= off[q.k] && q.end <= off[q.k + 1], "%s: g %d segment [%lld, %lld) leaves bucket %d",
            name, g, (long long)q.begin, (long long)q.end, q.k);
      if (q.begin > q.end || q.begin < 0 || q.end > L) continue;
      for (int64_t p = q.begin; p < q.end; ++p) ++seen[(size_t)p];
      steps += wgrad_steps(q.end - q.begin);
    }
    if (member) {  // the own range is the (slab, offset) range; members of a team are on one XCD label and distinct
      const int k = wgrad_member_offset(m_);
      CHECK(k != K / 2 && seg[0].k == k, "%s: g %d own bucket %d", name, g, seg[0].k);
      CHECK(seg[0].begin == off[k] + bd[t_ * K + k] && seg[0].end == off[k] + bd[(t_ + 1) * K + k], "%s: g %d own range", name, g);
      CHECK(g % kPlanXcd == t_ % kPlanXcd && wgrad_member_g(t_, m_) == g, "%s: g %d <-> (%d, %d)", name, g, t_, m_);
    }
    CHECK(seg[n - 1].k == K / 2, "%s: g %d last segment in bucket %d", name, g, seg[n - 1].k);
    smin = std::min(smin, steps);
    smax = std::max(smax, steps);
  }
  int64_t bad = 0;
  for (int64_t p = 0; p < L; ++p) bad += seen[(size_t)p] != 1;
  CHECK(bad == 0, "%s: %lld of %lld pair positions not covered exactly once", name, (long long)bad, (long long)L);
  std::printf("%-34s mode %d  L %9lld  steps per workgroup %lld .. %lld\n", name, mode, (long long)L, (long long)smin, (long long)smax);
  // the rule's claim: where AUTO takes the team sweep, every workgroup runs S or S - 1 steps
  if (mode == kTeamsAuto) CHECK(smax - smin <= 1, "%s: step counts differ by %lld under the rule", name, (long long)(smax - smin));
  return smax - smin;
}

// a hand-made table: sizes[k] pairs per bucket, cut[k](t) in [0, 1] ascending = the share of the bucket in front of slab t
template <typename F>
static Tables made_tables(const std::vector<int32_t>& sizes, F cut) {
  const int K = (int)sizes.size();
  Tables t;
  t.offsets.assign(K + 1, 0);
  t.bounds.assign((size_t)(kPlanSlabs + 1) * K, 0);
  for (int k = 0; k < K; ++k) {
    t.offsets[k + 1] = t.offsets[k] + sizes[k];
    for (int s = 0; s <= kPlanSlabs; ++s)
      t.bounds[(size_t)s * K + k] = s == 0 ? 0 : s == kPlanSlabs ? sizes[k] : (int32_t)(cut(k, s) * sizes[k]);
  }
  return t;
}

int main() {
  // ---- real small scenes (the shapes of tests/test_gpu_wgrad_teams.py), FORCE: they are far below the size condition ----
  struct { const char* name; int64_t n; int side; } scenes[] = {
      {"9600 voxels in 40^3", 9600, 40}, {"full 20^3 cube", 8000, 20}, {"4500 voxels in 64^3", 4500, 64},
      {"3000 voxels in 30^3", 3000, 30}, {"5001 voxels in 32^3", 5001, 32},   {"300 voxels in 12^3", 300, 12},
  };
  for (auto& s : scenes) {
    const Tables t = scene_tables(s.n, s.side, 7);
    check_tables(s.name, t, kTeamsForce, true);
    check_tables(s.name, t, kTeamsAuto, false);  // L < 512 x 512
  }
  // ---- a scene of the headline's kind, AUTO: the rule holds and the load is level to one step ----
  {
    const Tables t = scene_tables(400000, 150, 3);  // 12 % occupancy, as the headline scene
    const int64_t spread = check_tables("400 k voxels in 150^3 (auto)", t, kTeamsAuto, true);
    CHECK(spread >= 0 && spread <= 1, "step counts differ by %lld under the rule", (long long)spread);
    check_tables("400 k voxels in 150^3 (off)", t, kTeamsOff, false);
    Tables none = t;
    none.bounds.clear();
    check_tables("... without bounds", none, kTeamsForce, false);
  }
  // ---- adversarial tables ----
  std::mt19937 rng(11);
  auto even = [](int, int s) { return (double)s / kPlanSlabs; };
  {
    std::vector<int32_t> sz(27, 1000);
    for (int k : {0, 5, 13, 26}) sz[k] = 0;  // empty buckets, the centre among them
    check_tables("empty buckets", made_tables(sz, even), kTeamsForce, true);
    std::vector<int32_t> none(27, 0);
    check_tables("no pairs at all", made_tables(none, even), kTeamsForce, true);
  }
  {
    std::vector<int32_t> sz(27, 700);
    check_tables("empty slabs", made_tables(sz, [](int, int s) { return s < 9 ? 0.0 : s < 12 ? 0.5 : 1.0; }), kTeamsForce, true);
    check_tables("one slab per bucket", made_tables(sz, [](int k, int s) { return s <= k % 16 ? 0.0 : 1.0; }), kTeamsForce, true);
  }
  {
    std::vector<int32_t> sz(27, 9);
    sz[13] = 40;  // L = 274 < 512: most workgroups get nothing
    check_tables("L < 512", made_tables(sz, even), kTeamsForce, true);
    std::vector<int32_t> one(27, 0);
    one[3] = 1;
    check_tables("one pair", made_tables(one, even), kTeamsForce, true);
  }
  {
    std::vector<int32_t> sz(27, 20000);
    sz[13] = 300;  // a centre bucket far too small to level anything
    check_tables("tiny centre (auto)", made_tables(sz, even), kTeamsAuto, false);  // own ranges above the level: refused
    check_tables("tiny centre (force)", made_tables(sz, even), kTeamsForce, true);
    sz[13] = 120000;  // 96 / 512 of the pairs would be 120 000: the own ranges of 1 250 pairs sit exactly at the level
    check_tables("centre at the edge", made_tables(sz, even), kTeamsAuto, true);
    sz[13] = 110000;
    check_tables("centre below the edge", made_tables(sz, even), kTeamsAuto, false);
    sz[13] = 2000000;
    check_tables("huge centre", made_tables(sz, even), kTeamsAuto, true);
    sz[13] = 20000;
    sz[4] = 27000;  // 1.33 x the mean of the off-centre buckets
    check_tables("unbalanced (auto)", made_tables(sz, even), kTeamsAuto, false);
    check_tables("unbalanced (force)", made_tables(sz, even), kTeamsForce, true);
  }
  for (int trial = 0; trial < 40; ++trial) {  // random monotone tables
    std::vector<int32_t> sz(27);
    for (auto& v : sz) v = (rng() % 4 == 0) ? 0 : (int32_t)(rng() % (trial < 20 ? 3000 : 60000));
    std::vector<double> cuts((size_t)27 * (kPlanSlabs + 1));
    for (int k = 0; k < 27; ++k) {
      std::vector<double> c(kPlanSlabs + 1);
      for (auto& v : c) v = (rng() % 3 == 0) ? 0.0 : (double)(rng() % 1000) / 999.0;
      std::sort(c.begin(), c.end());
      for (int s = 0; s <= kPlanSlabs; ++s) cuts[(size_t)k * (kPlanSlabs + 1) + s] = c[s];
    }
    const std::string name = "random table " + std::to_string(trial);
    check_tables(name.c_str(), made_tables(sz, [&](int k, int s) { return cuts[(size_t)k * (kPlanSlabs + 1) + s]; }), kTeamsForce, true);
  }
  {  // what the rule must refuse whatever the mode: a table of other lists, another kernel volume, two tiles, another grid
    Tables t = scene_tables(3000, 30, 5);
    Tables stale = t;
    stale.bounds[(size_t)kPlanSlabs * 27 + 4] += 1;
    check_tables("stale table", stale, kTeamsForce, false);
    CHECK(!wgrad_team_rule(t.offsets.data(), t.bounds.data(), 27, kPlanGrid, 2, kTeamsForce), "two tiles");
    CHECK(!wgrad_team_rule(t.offsets.data(), t.bounds.data(), 27, 506, 1, kTeamsForce), "G = 506");
    CHECK(!wgrad_team_rule(t.offsets.data(), t.bounds.data(), 25, kPlanGrid, 1, kTeamsForce), "K = 25");
  }
  if (g_failures) {
    std::printf("%d checks FAILED\n", g_failures);
    return 1;
  }
  std::printf("all plan checks held\n");
  return 0;
}
