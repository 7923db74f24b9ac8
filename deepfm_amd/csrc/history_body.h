// The prior-set rule of the user histories (DESIGN.md §7b "User histories on the device"), stated once for the two
// kernels that form bags from the index of dfm_history_index_build:
//
//   history_gather_kernel    (history.hip)  materialises the bags of m queries;
//   record_assemble_kernel   (sampler.hip)  fills a bound SEQUENCE column of one batch record.
//
//   history_prior   per query: the first position of its user's segment and its prior count, under the three modes;
//   history_slot    per bag slot j: events[s + c - 1 - j] -> item row -> id, 0 past the count.
//
// Plain loads only.  Every index that comes out of memory is checked before it is used as one, so no read leaves its
// buffer whatever the index or the query holds.
#pragma once
#include "common.h"

namespace dfm {

struct HistoryIndex {
  const int64_t* users;
  const int64_t* items;
  const int64_t* ts;
  const int64_t* item_ids;       // NULL: item row + 1
  const int64_t* start;
  const int32_t* pos_of;
  const int32_t* rank;
  const int32_t* events;
  const int64_t* sorted_ts;
  const int32_t* event_count;
  int64_t n, n_users, n_items;
};

__device__ __forceinline__ bool history_inside(int64_t v, int64_t n) { return v >= 0 && v < n; }

// Query q (a log row; a user row for DFM_HISTORY_LATEST) -> *seg, the first position of its user's segment, and *c,
// its prior count, cut to the segment.  False, with both 0, for a query outside the log (the user table) or whose user
// row or position is outside the index.  `mode` is a constant in history_gather_kernel and folds there.  Keep the one
// exit and the two selects at the end: a form with early returns that stored its results on the way was miscompiled
// for a run-time `mode` (DESIGN.md §7b "History bags at record assembly").
__device__ __forceinline__ bool history_prior(const HistoryIndex& ix, int mode, int64_t q, int32_t* seg, int32_t* c) {
  int64_t u = -1, p = -1;
  if (mode == DFM_HISTORY_LATEST) {
    u = q;
  } else if (history_inside(q, ix.n)) {
    u = ix.users[q];
    p = ix.pos_of[q];
  }
  bool ok = history_inside(u, ix.n_users);
  int64_t s = 0, e = 0, prior = 0;
  if (ok) {
    s = ix.start[u];
    e = ix.start[u + 1];
    ok = s >= 0 && s <= e && e <= ix.n && (mode == DFM_HISTORY_LATEST || (p >= s && p < e));
  }
  if (ok) {
    if (mode == DFM_HISTORY_LATEST) {
      prior = ix.event_count[u];
    } else if (mode == DFM_HISTORY_POSITION) {
      prior = ix.rank[p];
    } else {                                             // the first position of [s, p] whose timestamp is not below t
      const int64_t t = ix.ts[q];
      int64_t lo = s, hi = p;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ix.sorted_ts[mid] < t) lo = mid + 1; else hi = mid;
      }
      prior = ix.rank[lo];
    }
    prior = prior < 0 ? 0 : (prior > e - s ? e - s : prior);        // whatever the index holds: inside the segment
  }
  *seg = ok ? static_cast<int32_t>(s) : 0;
  *c = ok ? static_cast<int32_t>(prior) : 0;
  return ok;
}

// Slot j >= 0 of the bag of a query with (seg, c) from history_prior: the id of its j-th latest prior event, 0 for
// j >= c.  *bad is set (and the id is 0) when the event row or its item row is outside its table.
__device__ __forceinline__ int64_t history_slot(const HistoryIndex& ix, int32_t seg, int32_t c, int j, bool* bad) {
  *bad = false;
  if (j >= c) return 0;
  const int64_t ev = ix.events[static_cast<int64_t>(seg) + c - 1 - j];
  const int64_t item = history_inside(ev, ix.n) ? ix.items[ev] : -1;
  if (!history_inside(item, ix.n_items)) {
    *bad = true;
    return 0;
  }
  return ix.item_ids ? ix.item_ids[item] : item + 1;
}

}  // namespace dfm
