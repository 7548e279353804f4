// greb_strip_order.cpp -- host only: the launch orders of the row-strip kernels on 384- and 192-wide grids.
//   step_rows_tasks   one circulation sub-step per launch (greb_step_rows.hip);
//   circ_rows_tasks   one circulation call per launch, with its dependency table (greb_circ_rows.hip);
//   rows_tasks        the batched diffusion sweep (greb_rows.hip).
// The two circulation orders are one schedule (deal_strips) under two descriptions of their form (StripForm).
// Speed only: every order covers each row of each field exactly once, and the results do not depend on it.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "greb_kernels.h"

namespace greb {
namespace {

// What a row costs, in cycles (tools/stamp_step_rows.py, tools/step_timeline.py; profiles/r03_g384_substep_*):
//   issue  the issue slots it takes on its SIMD -- one instruction per 4 cycles, shared by the SIMD's two wavefronts:
//          ~480 instructions for a streamed row, 36 per chain sweep (33 without the clamp minimum), ~210 to set a chain up;
//   wall   what the row takes a wavefront that has the SIMD to itself: a streamed row waits for memory (3 500 cycles for
//          1 900 of issue -- 2 200 as it shares the SIMD, the figure used), a chain never waits.
// Two strips on one SIMD end after max(their walls, the sum of their issues): measured 94 000 cycles for a polar strip of
// 63 500 beside a 16-row streaming strip (30 400 of issue), 61 000-70 000 for two such streaming strips.
struct RowCost { int issue, wall; };
constexpr int kRowIssue = 1900, kRowWall = 3500, kSweepCycles = 147, kChainSetupCycles = 850, kFillIssue = 700, kFillWall = 3800;

// the tuning knobs of the circulation orders (-DGREB_TUNING builds only; the release library has the constants)
struct OrderKnobs {
  int row_issue;    // a streamed row's issue (RowCost)
  int issue_pct;    // a strip's share of S in issue ...
  int wall_pct;     // ... and in wall time (measured: 1 member 19.1 us per launch at 85-100, 18.5 at 60-70)
  int chain_min;    // the one-launch form: rows with at least this many diffusion sweeps are chain tasks
  int chain_weight; // ... and their modelled cost in per cent (see circ_rows_tasks)
};
const OrderKnobs& knobs() {
  static const OrderKnobs k{tuning_int("GREB_STEP_ROWCOST", kRowIssue), tuning_int("GREB_STEP_ISSUE_PCT", 54),
                            tuning_int("GREB_STEP_WALL_PCT", 70), tuning_int("GREB_CIRC_CHAIN_MIN", kChainTaskMinSweeps),
                            tuning_int("GREB_CIRC_CHAIN_WEIGHT", 120)};
  return k;
}

RowCost step_row_cost(const RowTables& t, int k) {
  const int d = t.dif_time2[k], a = t.adv_time2[k];
  const int chains = (d > 1 ? kChainSetupCycles + kSweepCycles * d : 0) + (a > 1 ? kChainSetupCycles + kSweepCycles * a : 0);
  return {knobs().row_issue + chains, kRowWall + chains};
}

// a task of a circulation order: rows [k0, k1) of one (member, tracer) field
struct Strip { int field, k0, k1; long long issue, wall; bool chain; };

// Rows [a, b) of a field with row table t: as few strips as the two caps allow, cut where the cumulative issue crosses
// equal shares (a greedy cut leaves every strip some way below its cap: more strips, or a larger S, than needed)
void cut_rows(const RowTables& t, int a, int b, long long cap_issue, long long cap_wall, std::vector<Strip>& mine) {
  long long fi = 0, fw = 0;
  for (int k = a; k < b; ++k) { const RowCost c = step_row_cost(t, k); fi += c.issue; fw += c.wall; }
  const long long ci = std::max<long long>(1, cap_issue - kFillIssue), cw = std::max<long long>(1, cap_wall - kFillWall);
  const int n = (int)std::min<long long>(b - a, std::max((fi + ci - 1) / ci, (fw + cw - 1) / cw));
  long long acc = 0, issue = kFillIssue, wall = kFillWall;
  int start = a, cut = 1;
  for (int k = a; k < b; ++k) {
    const RowCost c = step_row_cost(t, k);
    // the share boundary cut * fi / n lies nearer the start of row k than its end: close the strip before it
    if (k > start && cut < n && 2 * n * acc + (long long)n * c.issue >= 2 * fi * cut) {
      mine.push_back({0, start, k, issue, wall, false});
      start = k; issue = kFillIssue; wall = kFillWall;
      while (cut < n && 2 * n * acc + (long long)n * c.issue >= 2 * fi * cut) ++cut; // (a dear row may span shares)
    }
    acc += c.issue; issue += c.issue; wall += c.wall;
  }
  mine.push_back({0, start, b, issue, wall, false});
}

// What tells the two circulation forms' orders apart
struct StripForm {
  int chain_min;    // rows with at least this many diffusion sweeps are tasks of one row (INT_MAX: none, whole fields are cut)
  int chain_weight; // per cent: a chain task's modelled cost against its sweeps and set-up
  int budget;       // at most this many tasks
  int passes;       // S is raised at most passes - 1 times ...
  bool must_fit;    // ... after which an order over budget is dropped (no tasks) or launched as it is
  bool rotate;      // the second round is dealt as the hardware seats a compute unit's second workgroup
};

// The launch order of one circulation sub-step or call.  The chip has slots / 2 SIMDs with two wavefront slots each (187
// VGPRs, 19.5 KB of LDS per wavefront); workgroup i of a launch lands on SIMD i mod (slots / 2), so tasks i and i + slots / 2
// share one.  A launch is as long as its longest SIMD, and a task started late -- because there are more tasks than slots
// -- runs its full length after the others are done (62 members as 2 388 tasks for 2 048 slots: 40 us, 13 of them for the
// 340 late strips).  So ONE round: the rows of all fields are cut into at most `budget` tasks such that a SIMD's pair ends
// after S cycles -- each strip at most S / 2 of issue and S of wall (RowCost) -- with S the smallest that fits, but no
// less than the dearest row's wall (the 232-sweep polar row: few fields gain nothing from strips that end before it).
// With n tasks for n_simd SIMDs, n - n_simd SIMDs hold a pair: the tasks with the most issue run alone, the others are
// paired dearest with cheapest (two chain strips on one SIMD -- both issue without a pause -- take twice as long each).
std::vector<Strip> deal_strips(const RowTables* tabs, const int* tab_index, int n_members, int ny, int n_slots,
                               const StripForm& form) {
  const int n_simd = std::max(1, n_slots / 2);
  auto is_chain = [&](const RowTables& t, int k) { return t.dif_time2[k] >= form.chain_min; };
  // a chain task: its sweeps and set-up, the meridional part, no streaming
  auto chain_cost = [&](const RowTables& t, int k) {
    const RowCost c = step_row_cost(t, k);
    return (long long)(c.issue - kRowIssue + 800) * form.chain_weight / 100;
  };
  long long total = 0, dearest = 0;
  for (int m = 0; m < n_members; ++m)
    for (int k = 0; k < ny; ++k) {
      const RowTables& t = tabs[tab_index[m]];
      const RowCost c = step_row_cost(t, k);
      total += 2 * (is_chain(t, k) ? chain_cost(t, k) : c.issue);
      dearest = std::max<long long>(dearest, is_chain(t, k) ? chain_cost(t, k) : c.wall + kFillWall);
    }
  long long S = std::max(total / n_simd, dearest);
  const int issue_pct = knobs().issue_pct, wall_pct = knobs().wall_pct;
  std::vector<Strip> all;
  for (int pass = 0;; ++pass) {
    const long long cap_issue = S * issue_pct / 100, cap_wall = S * wall_pct / 100;
    all.clear();
    for (int m = 0; m < n_members; ++m) {
      const RowTables& t = tabs[tab_index[m]];
      std::vector<Strip> mine;
      int a = 0;
      for (int k = 0; k <= ny; ++k) { // the rows between two chain rows as strips, every chain row a task of its own
        if (k < ny && !is_chain(t, k)) continue;
        if (k > a) cut_rows(t, a, k, cap_issue, cap_wall, mine);
        if (k < ny) mine.push_back({0, k, k + 1, chain_cost(t, k), chain_cost(t, k), true});
        a = k + 1;
      }
      for (int tr = 0; tr < 2; ++tr)
        for (Strip x : mine) { x.field = 2 * m + tr; all.push_back(x); }
    }
    if ((int)all.size() <= form.budget) break;
    if (pass + 1 == form.passes) {
      if (form.must_fit) return {}; // (cannot happen for ny <= 192: one strip per segment is reached long before)
      break;
    }
    S += S / 40;
  }
  std::stable_sort(all.begin(), all.end(), [](const Strip& x, const Strip& y) { return x.issue > y.issue; });
  const int n_all = (int)all.size();
  if (n_all > n_simd && n_all <= 2 * n_simd) {
    const int m = n_all - n_simd, alone = n_simd - m; // m SIMDs hold a pair
    std::vector<Strip> order((size_t)n_all);
    for (int j = 0; j < m; ++j) {
      order[(size_t)j] = all[(size_t)(alone + j)];                // the dearer of pair j ...
      order[(size_t)(n_simd + j)] = all[(size_t)(n_all - 1 - j)]; // ... and the cheapest left
    }
    for (int j = 0; j < alone; ++j) order[(size_t)(m + j)] = all[(size_t)j];
    // ... as the hardware deals them: the wavefronts of the SECOND workgroup on a compute unit start one SIMD further on
    // (observed, tools/circ_timeline.py: second-round wavefront w sits on SIMD (w + 1) mod 4, so task i shares its SIMD
    // with task i + 1 023 or i + 1 027, never i + 1 024): the partner meant for SIMD w goes to wavefront (w + 3) mod 4
    for (int c = 0; form.rotate && n_simd + 4 * c + 3 < n_all; ++c) {
      const size_t b = (size_t)n_simd + 4 * (size_t)c;
      const Strip t0 = order[b], t1 = order[b + 1], t2 = order[b + 2], t3 = order[b + 3];
      order[b + 3] = t0; order[b] = t1; order[b + 1] = t2; order[b + 2] = t3;
    }
    all.swap(order);
  }
  return all;
}

int strip_cost(int time2) { return time2 > 1 ? 130 + 36 * time2 : 120; }

struct CapStrip { int k0, k1, cost, up; };

// contiguous strips of about `target` instructions over rows [ka, kb), never splitting a row; a strip is closed when
// the next row would take it over the target, unless it is still tiny
void cut_strips(const RowTables& t, int ka, int kb, int target, std::vector<CapStrip>& out) {
  int acc = 0, start = ka;
  for (int k = ka; k < kb; ++k) {
    const int cst = strip_cost(t.dif_time2[k]);
    if (acc > 0 && acc + cst > target && acc >= 600) { out.push_back({start, k, acc, 0}); start = k; acc = 0; }
    acc += cst;
  }
  if (kb > ka) out.push_back({start, kb, acc, 0});
}

} // namespace

bool step_rows_supported(const RowTables* tabs, int n_tabs, int nx, int ny) {
  // a row fills the wavefront's 384 longitudes once or twice (greb_rows.h)
  if ((nx != 384 && nx != 192) || ny < 5 || ny > kMaxNy) return false;
  for (int t = 0; t < n_tabs; ++t)
    for (int k = 0; k < ny; ++k)
      if (!tabs[t].subcycled[k] || tabs[t].dif_time2[k] < 1 || tabs[t].adv_time2[k] < 1) return false;
  return true;
}

// One launch per sub-step: whole fields are cut into at most two tasks per SIMD -- or, should that not be reached, the
// last cut is launched as it is (no task waits for another: a late one only ends the launch late).
void step_rows_tasks(const RowTables* tabs, const int* tab_index, int n_members, int ny, int n_slots,
                     std::vector<RowsTask>& tasks) {
  const int n_simd = std::max(1, n_slots / 2);
  const std::vector<Strip> all = deal_strips(tabs, tab_index, n_members, ny, n_slots, {INT_MAX, 100, 2 * n_simd, 96, false, false});
  tasks.clear();
  tasks.reserve(all.size());
  for (const Strip& x : all) tasks.push_back({x.field | (tab_index[x.field >> 1] << kStepFieldBits), x.k0 | (x.k1 << 8) | kRowsUp});
}

// the launch order on the device (owned by the caller: the engine keeps one per member count and frees it with itself)
hipError_t step_rows_make_tasks(const RowTables* tabs_host, const int* tab_index_host, int n_members, int ny,
                                int n_slots, RowsTask** dev, int* n, RowsTask* head) {
  std::vector<RowsTask> host;
  step_rows_tasks(tabs_host, tab_index_host, n_members, ny, n_slots, host);
  for (int i = 0; i < kStepHeadTasks; ++i) head[i] = i < (int)host.size() ? host[(size_t)i] : RowsTask{0, 0};
  hipError_t e = hipMalloc(dev, host.size() * sizeof(RowsTask));
  if (e != hipSuccess) return e;
  if ((e = hipMemcpy(*dev, host.data(), host.size() * sizeof(RowsTask), hipMemcpyHostToDevice)) != hipSuccess) {
    (void)hipFree(*dev);
    *dev = nullptr;
    return e;
  }
  *n = (int)host.size();
  return hipSuccess;
}

// One launch per circulation call: per field the chain rows (one task each) and, between them, strips -- at most n_slots
// tasks in all, every one resident at once (no order otherwise), the second round rotated as the hardware seats it.  A
// chain task on a shared SIMD is the one that never waits (tools/circ_timeline.py), so its cost is weighted up: it is
// dealt the cheaper partner.  Then every task's dependencies: the owners of the two rows below and the two rows above
// its own.
void circ_rows_tasks(const RowTables* tabs, const int* tab_index, int n_members, int ny, int n_slots,
                     std::vector<CircTask>& tasks) {
  const std::vector<Strip> all = deal_strips(tabs, tab_index, n_members, ny, n_slots,
                                             {knobs().chain_min, knobs().chain_weight, n_slots, 200, true, true});
  const int n_all = (int)all.size();
  tasks.clear();
  // who owns which row of which field
  std::vector<int> owner((size_t)2 * n_members * ny, -1);
  for (int i = 0; i < n_all; ++i)
    for (int k = all[(size_t)i].k0; k < all[(size_t)i].k1; ++k) owner[(size_t)all[(size_t)i].field * ny + k] = i;
  tasks.reserve((size_t)n_all);
  for (int i = 0; i < n_all; ++i) {
    const Strip& x = all[(size_t)i];
    CircTask c{x.field | (tab_index[x.field >> 1] << kStepFieldBits), x.k0 | (x.k1 << 8) | kRowsUp | (x.chain ? kCircChain : 0),
               {-1, -1, -1, -1}, (int)std::min<long long>(x.issue, 0x7fffffff), 0};
    int nd = 0;
    const int near[4] = {x.k0 - 2, x.k0 - 1, x.k1, x.k1 + 1};
    for (int j = 0; j < 4; ++j) {
      if (near[j] < 0 || near[j] >= ny) continue;
      const int o = owner[(size_t)x.field * ny + near[j]];
      if (o == i) continue;
      bool seen = false;
      for (int q = 0; q < nd; ++q) seen = seen || c.dep[q] == o;
      if (!seen) c.dep[nd++] = o;
    }
    tasks.push_back(c);
  }
}

hipError_t circ_rows_make_order(const RowTables* tabs_host, const int* tab_index_host, int n_members, int ny, int n_slots,
                                CircOrder* out) {
  std::vector<CircTask> host;
  circ_rows_tasks(tabs_host, tab_index_host, n_members, ny, n_slots, host);
  *out = CircOrder{};
  if (host.empty() || (int)host.size() > n_slots) return hipSuccess; // n == 0: the caller takes one launch per sub-step
  hipError_t e = hipMalloc(&out->tasks, host.size() * sizeof(CircTask));
  if (e == hipSuccess) e = hipMalloc(&out->flags, host.size() * sizeof(unsigned));
  if (e == hipSuccess) e = hipMalloc(&out->ctrl, 8 * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemcpy(out->tasks, host.data(), host.size() * sizeof(CircTask), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(out->flags, 0, host.size() * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemset(out->ctrl, 0, 8 * sizeof(unsigned));
  if (e != hipSuccess) { circ_rows_free_order(out); return e; }
  out->n = (int)host.size();
  out->epoch = 0;
  return hipSuccess;
}

void circ_rows_free_order(CircOrder* o) {
  if (o->tasks) (void)hipFree(o->tasks);
  if (o->flags) (void)hipFree(o->flags);
  if (o->ctrl) (void)hipFree(o->ctrl);
  *o = CircOrder{};
}

int circ_rows_status(const CircOrder& o, unsigned* diag5) {
  unsigned h[8] = {0};
  if (!o.ctrl) return 0;
  if (hipMemcpy(h, o.ctrl, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -2;
  if (diag5) std::memcpy(diag5, h + 1, 5 * sizeof(unsigned));
  return h[0] ? -1 : 0;
}

// The launch order of the diffusion sweep.  Two kinds of task: CHAIN strips (the rows next to the poles that iterate:
// arithmetic, a lone wavefront issuing one instruction per ~5 cycles) and STREAMING strips (the single-sweep rows between
// the caps: memory).
//   * they are interleaved, the chain strips spread evenly over the first `chain_span` per cent of the launch: at any
//     moment a SIMD holds about one chain wave beside streaming ones, so the arithmetic hides under the traffic
//     (dearest-first order ran the chains first and the traffic after them: 0.210 ms against 0.190);
//   * the streaming region is cut into few long strips for most fields (halo rows re-read: 2 per strip) and into ever
//     shorter ones for the fields launched last (levels below): when the last task starts, what is still running is
//     small, so the launch does not end on a handful of wavefronts each streaming at its own latency-bound ~3 GB/s;
//   * tasks come in groups of eight (the same strip of eight consecutive fields): blocks are dealt to the eight XCDs in
//     turn, so all strips of a field run on one XCD, and neighbouring strips walk away from their common border (one
//     down, one up): the halo rows both read are requested together and the second reader finds them in that XCD's L2.
// Speed only: any order gives the same result bit for bit, every row is written by exactly one task.
void rows_tasks(const RowTables& t, int ny, int batch, const RowsTuning& tu, std::vector<RowsTask>& tasks) {
  // the streaming region: the run of single-sweep rows around the equator
  int ks = ny / 2, ke = ny / 2;
  while (ks > 0 && t.dif_time2[ks - 1] == 1) --ks;
  while (ke < ny && t.dif_time2[ke] == 1) ++ke;
  if (t.dif_time2[ny / 2] != 1) ks = ke = ny / 2; // (no such run: everything is a chain strip)
  std::vector<CapStrip> caps;
  cut_strips(t, 0, ks, tu.chain_target, caps);
  cut_strips(t, ke, ny, tu.chain_target, caps);
  for (size_t i = 0; i < caps.size(); ++i) caps[i].up = (int)(i & 1);
  std::stable_sort(caps.begin(), caps.end(), [](const CapStrip& x, const CapStrip& y) { return x.cost > y.cost; });
  const int G = (batch + 7) / 8, len = ke - ks;
  // levels of the streaming cut, coarse to fine; the finer levels take the LAST groups of fields
  int parts[4], first[5];
  for (int l = 0; l < 4; ++l) parts[l] = std::max(1, std::min(len, tu.parts[l]));
  first[4] = G;
  for (int l = 3; l >= 1; --l) {
    const int groups = len > 0 ? (tu.level_tasks[l] + 8 * parts[l] - 1) / (8 * parts[l]) : 0;
    first[l] = std::max(0, first[l + 1] - groups);
  }
  first[0] = 0;
  struct Oct { double pos; int group, k0, k1, up; };
  std::vector<Oct> so, co;
  double sw = 0, cw = 0;
  if (len > 0)
    for (int l = 0; l < 4; ++l)
      for (int g = first[l]; g < first[l + 1]; ++g)
        for (int i = 0; i < parts[l]; ++i) {
          const int a0 = ks + (int)((long long)len * i / parts[l]), a1 = ks + (int)((long long)len * (i + 1) / parts[l]);
          so.push_back({sw, g, a0, a1, i & 1});
          sw += a1 - a0 + 2;
        }
  for (int g = 0; g < G; ++g)
    for (const CapStrip& c : caps) { co.push_back({cw, g, c.k0, c.k1, c.up}); cw += c.cost; }
  for (Oct& o : so) o.pos /= sw > 0 ? sw : 1;
  const double span = so.empty() ? 1.0 : tu.chain_span * 0.01;
  for (Oct& o : co) o.pos *= span / (cw > 0 ? cw : 1);
  std::vector<Oct> all(so.size() + co.size());
  std::merge(co.begin(), co.end(), so.begin(), so.end(), all.begin(), [](const Oct& x, const Oct& y) { return x.pos < y.pos; });
  tasks.clear();
  tasks.reserve(all.size() * 8);
  for (const Oct& o : all)
    for (int f = 0; f < 8; ++f) {
      const int field = 8 * o.group + f;
      tasks.push_back({field < batch ? field : -1, o.k0 | (o.k1 << 8) | (o.up ? kRowsUp : 0)});
    }
}

} // namespace greb
