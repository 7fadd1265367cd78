// wgrad_plan.h - which pairs a workgroup of the weight-gradient launch sweeps: plain integer code, compiled for the
// host (tests, wcn_wgrad_plan_host) and for the device (wgrad_mfma.hip) from this one text.
//
// Two sweeps exist.  The RANGE sweep cuts the concatenated pair list [0, L) into G equal contiguous ranges; it takes any
// map.  The TEAM sweep needs `bounds` - int32 [kPlanSlabs + 1][K], bounds[t][k] = pairs of bucket k whose output row
// lies in front of row slab t (T = 16 slabs of ceil(ntile / 16) 256-row tiles; written by the kernel-map scan, in-bucket
// positions, bounds[0][k] = 0, bounds[16][k] = the bucket's size) - and a 3 x 3 x 3 map:
//
//   * team t = slab t; its K - 1 = 26 members are the workgroups g with g % 8 == t % 8 (the XCD a workgroup most
//     likely lands on; an affinity, nothing depends on it) that wgrad_member() names, one per off-centre offset;
//   * member (t, k) sweeps [bounds[t][k], bounds[t + 1][k]) of bucket k: buckets are ordered by output row, so the 26
//     members walk the same dY rows from the same start at the same pair rate and 25 of 26 gathers of a row can hit L2;
//   * the centre bucket (pairs (r, r): streamed, nothing to reuse) levels the load: in 64-pair steps, every workgroup is
//     filled up to S0 (the first `r` workgroups) or S0 - 1 steps with a piece of it, pieces in ascending g;
//   * workgroup g flushes its own range to slab 2g and its centre piece to slab 2g + 1, empty ones as zero tiles.
//
// Nothing here waits for, counts or looks at another workgroup; a table that is not monotone costs coverage of that
// map's own result, never an access outside a bucket (every bound is clamped to its bucket).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WCN_PLAN_FN __host__ __device__ inline
#else
#define WCN_PLAN_FN inline
#endif

namespace wcn {

constexpr int kPlanSlabs = 16;   // T: row slabs = teams
constexpr int kPlanGrid = 512;   // G of a team launch
constexpr int kPlanK = 27;       // 3 x 3 x 3, centre bucket at 13
constexpr int kPlanXcd = 8;      // workgroup g is expected on XCD g % 8
constexpr int kPlanStep = 64;    // pairs per pipeline step (kPairs)
constexpr int kPlanMembers = kPlanK - 1;
enum { kTeamsOff = 0, kTeamsAuto = 1, kTeamsForce = 2 };

struct WgradSeg {
  int k;
  int64_t begin, end;  // positions in the concatenated pair list; begin == end: nothing to sweep (a zero tile is flushed)
};

// The rule, first part (what one thread evaluates from offsets[] and the edges of the table; the second part is
// wgrad_level_holds): does this launch take the team sweep?  Every workgroup of wgrad_mfma_kernel evaluates both parts on the
// same operands and the reduce kernel reads the outcome.
WCN_PLAN_FN bool wgrad_team_rule(const int32_t* offsets, const int32_t* bounds, int K, int G, int tiles, int mode) {
  if (mode == kTeamsOff || !bounds || K != kPlanK || G != kPlanGrid || tiles != 1) return false;
  // (the size first: one word, and most launches of a network end here)
  if (mode != kTeamsForce && (int64_t)offsets[K] - offsets[0] < (int64_t)512 * G) return false;  // >= 512 pairs per workgroup
  // (a fixed trip count and no exit inside the loop: on the device all 4 x 27 loads are requested at once - with an early
  // return every iteration was a round trip of its own, 25 us in front of both kernels)
  int64_t off_sum = 0, off_max = 0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < kPlanK; ++k) {
    const int64_t cnt = (int64_t)offsets[k + 1] - offsets[k];
    // the table belongs to these lists: it starts every bucket at 0 and ends it at the bucket's size
    ok = ok & (cnt >= 0) & (bounds[k] == 0) & (bounds[kPlanSlabs * kPlanK + k] == cnt);
    if (k != kPlanK / 2) {
      off_sum += cnt;
      off_max = cnt > off_max ? cnt : off_max;
    }
  }
  if (!ok) return false;
  if (mode == kTeamsForce) return true;
  return off_max * (K - 1) * 10 <= off_sum * 11;          // largest off-centre bucket <= 1.10 x their mean
}

// member (team t, off-centre index m in [0, 26)) <-> workgroup
WCN_PLAN_FN int wgrad_member_g(int t, int m) { return (t % kPlanXcd) + kPlanXcd * ((t / kPlanXcd) * kPlanMembers + m); }
WCN_PLAN_FN bool wgrad_member(int g, int* t, int* m) {
  const int x = g % kPlanXcd, j = g / kPlanXcd;
  if (j >= 2 * kPlanMembers) return false;  // the remaining workgroups sweep centre pieces only
  *t = x + kPlanXcd * (j / kPlanMembers);
  *m = j % kPlanMembers;
  return true;
}
WCN_PLAN_FN int wgrad_member_offset(int m) { return m < kPlanK / 2 ? m : m + 1; }

WCN_PLAN_FN int64_t plan_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// own range of workgroup g (empty for the centre-only workgroups): false if g is no member
WCN_PLAN_FN bool wgrad_own_range(const int32_t* offsets, const int32_t* bounds, int K, int g, WgradSeg* seg) {
  int t, m;
  seg->k = K / 2;
  seg->begin = seg->end = offsets[K / 2];
  if (!wgrad_member(g, &t, &m)) return false;
  const int k = wgrad_member_offset(m);
  const int64_t cnt = (int64_t)offsets[k + 1] - offsets[k];
  const int64_t lo = plan_clamp(bounds[t * K + k], cnt);
  int64_t hi = plan_clamp(bounds[(t + 1) * K + k], cnt);
  if (hi < lo) hi = lo;
  seg->k = k;
  seg->begin = offsets[k] + lo;
  seg->end = offsets[k] + hi;
  return true;
}

WCN_PLAN_FN int64_t wgrad_steps(int64_t pairs) { return (pairs + kPlanStep - 1) / kPlanStep; }

WCN_PLAN_FN int64_t wgrad_own_steps(const int32_t* offsets, const int32_t* bounds, int K, int g) {
  WgradSeg s;
  wgrad_own_range(offsets, bounds, K, g, &s);
  return wgrad_steps(s.end - s.begin);
}

// the level: steps workgroup g runs when the centre pieces can fill every workgroup up to it (own_total = the steps of all
// own ranges together)
WCN_PLAN_FN int64_t wgrad_level(int64_t centre_pairs, int64_t own_total, int G, int g) {
  const int64_t n = wgrad_steps(centre_pairs) + own_total;  // steps of the whole launch
  const int64_t s0 = (n + G - 1) / G;
  const int64_t r = n - (s0 - 1) * G;                       // workgroups [0, r) run s0 steps, the others s0 - 1
  return g < r ? s0 : s0 - 1;
}

// steps of the centre bucket workgroup g takes
WCN_PLAN_FN int64_t wgrad_centre_steps(int64_t centre_pairs, int64_t own_total, int64_t own_steps, int G, int g) {
  const int64_t target = wgrad_level(centre_pairs, own_total, G, g);
  return target > own_steps ? target - own_steps : 0;
}

// Second part of the rule (AUTO only; FORCE drops it with the other size and balance conditions): no own range is longer than
// its workgroup's level - an own range cannot be cut, so a longer one (a centre bucket with less than about 96 / 512 of the
// pairs: dense volumes; rows whose density differs from slab to slab) would leave the launch unlevel.  Where it holds every
// workgroup runs S or S - 1 steps.  On the device the workgroup evaluates it together (two g per thread, one vote).
WCN_PLAN_FN bool wgrad_level_holds(int64_t centre_pairs, int64_t own_total, int64_t own_steps, int G, int g) {
  return own_steps <= wgrad_level(centre_pairs, own_total, G, g);
}

// The whole rule, serially (host)
WCN_PLAN_FN bool wgrad_team_rule_all(const int32_t* offsets, const int32_t* bounds, int K, int G, int tiles, int mode) {
  if (!wgrad_team_rule(offsets, bounds, K, G, tiles, mode)) return false;
  if (mode == kTeamsForce) return true;
  const int64_t centre = (int64_t)offsets[K / 2 + 1] - offsets[K / 2];
  int64_t own_total = 0;
  for (int q = 0; q < G; ++q) own_total += wgrad_own_steps(offsets, bounds, K, q);
  for (int q = 0; q < G; ++q)
    if (!wgrad_level_holds(centre, own_total, wgrad_own_steps(offsets, bounds, K, q), G, q)) return false;
  return true;
}

// the centre piece from its place in the ascending-g order (`before` = centre steps of the workgroups in front of g)
WCN_PLAN_FN void wgrad_centre_piece(const int32_t* offsets, int K, int64_t before, int64_t steps, WgradSeg* seg) {
  const int64_t c0 = offsets[K / 2], cnt = (int64_t)offsets[K / 2 + 1] - c0;
  seg->k = K / 2;
  seg->begin = c0 + plan_clamp(before * kPlanStep, cnt);
  seg->end = c0 + plan_clamp((before + steps) * kPlanStep, cnt);
}

// The whole plan of workgroup g, serially (host; the kernel forms the two sums with a block reduction instead).
// -> number of segments: seg[0] = own range (members only), seg[last] = centre piece.  Segment s flushes to slab 2g + s
// for members; a centre-only workgroup has one segment, which flushes to slab 2g + 1.
WCN_PLAN_FN int wgrad_team_plan(const int32_t* offsets, const int32_t* bounds, int K, int G, int g, WgradSeg seg[2]) {
  const int64_t centre = (int64_t)offsets[K / 2 + 1] - offsets[K / 2];
  int64_t own_total = 0;
  for (int q = 0; q < G; ++q) own_total += wgrad_own_steps(offsets, bounds, K, q);
  int64_t before = 0;
  for (int q = 0; q < g; ++q)
    before += wgrad_centre_steps(centre, own_total, wgrad_own_steps(offsets, bounds, K, q), G, q);
  const bool member = wgrad_own_range(offsets, bounds, K, g, &seg[0]);
  const int64_t own = wgrad_steps(seg[0].end - seg[0].begin);
  wgrad_centre_piece(offsets, K, before, wgrad_centre_steps(centre, own_total, own, G, g), &seg[member ? 1 : 0]);
  return member ? 2 : 1;
}

}  // namespace wcn
