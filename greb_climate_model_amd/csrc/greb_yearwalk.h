// greb_yearwalk.h -- what greb_cross and greb_reg share in following a yearly quantity of the records: the table of a plan's
// items (events, terms) as the update kernels walk them, its builder and its check on the host, and the walk itself on the
// device.  A model year is [member][12][n_vars][np]; an item is a selector (greb_season.h) of one variable, of the member
// or of the member minus its control (`rel`).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "greb_season.h"

namespace greb {

// The items sorted by variable, then by selector: those of distinct variable v are item[vstart[v]] ... item[vstart[v + 1] - 1].
// An Item has `sel`, `rel` and `out`, its index in the caller's order: where its state and products lie.  Travels by value
// in the kernel arguments and is read through the scalar cache.
template <class Item_, int N>
struct YearTable {
  using Item = Item_;
  Item item[N];
  int n_vars_used;   // distinct variables among the items
  int var[N];        // [n_vars_used] the variable
  int vstart[N + 1]; // [n_vars_used + 1]
  int months[N];     // [n_vars_used] bit mo: the variable's items need month mo of the member
  int ctl_months[N]; // ... of the member's control (the months of the `rel` items)
  int rel_sels[N];   // [n_vars_used] bit s: an item with selector s is `rel`
};

// The table of n items given in the caller's order (src[i] has `var`, `sel`, `rel`; the caller's order among equals).
// `fill(item, src[i])` sets what an Item has beyond sel, rel and out.
template <class Item, int N, class Src, class Fill>
void build_year_table(YearTable<Item, N>& t, const Src* src, int n, Fill fill) {
  int order[N];
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order, order + n, [src](int a, int b) { return src[a].var != src[b].var ? src[a].var < src[b].var : src[a].sel < src[b].sel; });
  t = YearTable<Item, N>{};
  int v = -1;
  for (int i = 0; i < n; ++i) {
    const Src& s = src[order[i]];
    t.item[i].sel = s.sel; t.item[i].rel = s.rel; t.item[i].out = order[i];
    fill(t.item[i], s);
    if (v < 0 || t.var[v] != s.var) { ++v; t.var[v] = s.var; t.vstart[v] = i; }
    t.months[v] |= season::months_of(s.sel);
    if (s.rel) { t.ctl_months[v] |= season::months_of(s.sel); t.rel_sels[v] |= 1 << s.sel; }
  }
  t.n_vars_used = v + 1;
  t.vstart[t.n_vars_used] = n;
}

// What the walk indexes with: nothing may point outside the records [.][12][n_vars][np] or the state [.][n_items][np].
template <class Item, int N>
bool year_table_ok(const YearTable<Item, N>& t, int n_vars, int n_items, bool has_control) {
  if (n_items < 1 || n_items > N || t.n_vars_used < 1 || t.n_vars_used > n_items || t.vstart[0] != 0 || t.vstart[t.n_vars_used] != n_items)
    return false;
  for (int v = 0; v < t.n_vars_used; ++v) {
    if (t.var[v] < 0 || t.var[v] >= n_vars || t.vstart[v + 1] <= t.vstart[v] || t.vstart[v + 1] > n_items) return false;
    for (int i = t.vstart[v]; i < t.vstart[v + 1]; ++i) {
      const Item& it = t.item[i];
      if (it.sel < 0 || it.sel >= season::kSelectors || it.out < 0 || it.out >= n_items || (i > t.vstart[v] && it.sel < t.item[i - 1].sel)) return false;
      const int months = season::months_of(it.sel);
      if ((months & ~t.months[v]) || (it.rel && (!has_control || (months & ~t.ctl_months[v]) || !(t.rel_sels[v] >> it.sel & 1)))) return false;
    }
  }
  return true;
}

// The body of an update kernel of grid (blocks of THREADS point quads, member, distinct variable).  A lane owns four
// consecutive points.  It loads the months its variable's items need -- the month mask is wave-uniform and decided by scalar
// branches -- as 16-byte vectors, the control's too where an item is `rel`, so that every record byte is read once as the
// member's own data and at most once as a control however many items share the variable.  Then it walks the variable's items
// (a uniform loop over the table): the quantity of a selector is formed once, and each(item, g, q) gets every item with
// g = the quad's index in [member][n_items][np / 4] and q = its quantity, a quiet NaN for a `rel` item of a member without
// a control.
template <int THREADS, class Table, class Each>
__device__ inline void year_walk(const Table& t, const float* x_all, const int* control, size_t np, int n_vars, int n_items, Each each) {
  using season::f4;
  using season::kMonths;
  using season::quantity;
  const size_t gp = np >> 2, quad = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (quad >= gp) return;
  const int m = (int)blockIdx.y, v = (int)blockIdx.z;
  const int var = t.var[v], own = t.months[v], rel_sels = t.rel_sels[v];
  const int c = control ? control[m] : -1;
  const int ctl = c >= 0 ? t.ctl_months[v] : 0;
  const size_t mon = (size_t)n_vars * gp; // quads of one month of one member
  const f4* xm = reinterpret_cast<const f4*>(x_all) + ((size_t)m * kMonths * n_vars + var) * gp + quad;
  const f4* xc = reinterpret_cast<const f4*>(x_all) + ((size_t)(c >= 0 ? c : 0) * kMonths * n_vars + var) * gp + quad;
  f4 x[kMonths], y[kMonths];
#pragma unroll
  for (int mo = 0; mo < kMonths; ++mo) {
    x[mo] = f4{0.f, 0.f, 0.f, 0.f};
    if (own >> mo & 1) x[mo] = xm[mo * mon];
  }
#pragma unroll
  for (int mo = 0; mo < kMonths; ++mo) {
    y[mo] = f4{0.f, 0.f, 0.f, 0.f};
    if (ctl >> mo & 1) y[mo] = xc[mo * mon];
  }
  const float nan = __builtin_nanf("");
  const f4 nan4 = {nan, nan, nan, nan};
  int i = t.vstart[v];
  const int end = t.vstart[v + 1];
#pragma unroll
  for (int s = 0; s < season::kSelectors; ++s) {
    if (i >= end || t.item[i].sel != s) continue; // (uniform)
    const f4 own_a = quantity(s, x);
    f4 rel_q = nan4;
    if ((rel_sels >> s & 1) && c >= 0) rel_q = own_a - quantity(s, y); // ONE fp32 subtraction
    for (; i < end && t.item[i].sel == s; ++i) {
      const typename Table::Item it = t.item[i];
      each(it, ((size_t)m * n_items + it.out) * gp + quad, it.rel ? rel_q : own_a);
    }
  }
}

} // namespace greb
