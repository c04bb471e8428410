// The conference table of the rate converter (include/percepnet_hip.h "conferences"), the rules that need no GPU, each stated once —
// HIP-free (builds with -DPN_NO_HIP), checked on the CPU by tests/c/conf_sanitize.cpp under the sanitizers and by
// tests/test_conf_host.py through the C-ABI: what a conference id must be, the table after a change, the member-count rule, and
// the members of a conference in ascending slot order — the order the mix kernel (pn_rate_mix.hip) adds them in.
// A table is one int32 per stream: PN_CONF_NONE, or the conference the stream is in, a number in [0, n_streams).
#pragma once
#include "pn_host_rules.h"   // pn_ids_check, pn_set_error, PN_CONF_NONE / PN_CONF_MAX_MEMBERS
#include <algorithm>

static inline bool pn_conf_value_ok(int32_t v, int n_streams) { return v == PN_CONF_NONE || (v >= 0 && v < n_streams); }

// confs[0..n): every one PN_CONF_NONE or in [0, n_streams).  -1 with pn_last_error naming the FIRST bad index; n == 0 is a legal list.
static inline int pn_conf_list_check(const int32_t *confs, int n, int n_streams) {
  if (n < 0 || n_streams < 0 || (n > 0 && !confs)) { pn_set_error("bad argument"); return -1; }
  for (int i = 0; i < n; i++)
    if (!pn_conf_value_ok(confs[i], n_streams)) {
      pn_set_error("conference %d at index %d: PN_CONF_NONE (%d) or a number in [0, %d)", (int)confs[i], i, PN_CONF_NONE, n_streams);
      return -1;
    }
  return 0;
}
// A change: ids[0..n) distinct streams of a batch of B (pn_ids_check), confs[i] the new conference of ids[i].
static inline int pn_conf_set_check(int B, const int32_t *ids, int n, const int32_t *confs) {
  if (pn_ids_check(B, ids, n, true)) return -1;
  return pn_conf_list_check(confs, n, B);
}

// The members of conference c in `table`, ascending, into out[0..PN_CONF_MAX_MEMBERS); returns how many the table holds (which a
// table that passed pn_conf_change never has above the cap; only the first PN_CONF_MAX_MEMBERS are written).
static inline int pn_conf_members(const std::vector<int32_t> &table, int32_t c, int32_t *out) {
  int k = 0;
  for (size_t s = 0; s < table.size(); s++)
    if (table[s] == c && c != PN_CONF_NONE) { if (k < PN_CONF_MAX_MEMBERS) out[k] = (int32_t)s; k++; }
  return k;
}

// What a change makes of a table, all of it decided before anything is launched.
struct PnConfChange {
  std::vector<int32_t> next;      // [B] the table after the change
  std::vector<int32_t> touched;   // the conferences a stream leaves or joins, ascending, each once
  std::vector<int32_t> rows;      // [touched][PN_CONF_MAX_MEMBERS] their members in `next`, ascending, padded with -1
  int in_conf = 0;                // streams of `next` that are in a conference
};
// cur: the table now ([B]).  0 with *ch filled; -1 with pn_last_error set and *ch unspecified for a bad or duplicate id, a bad value,
// or a conference that would hold more than PN_CONF_MAX_MEMBERS streams AFTER the change (the lowest such conference is named, with
// its size) — so one call may move streams between two full conferences in both directions.
static inline int pn_conf_change(const std::vector<int32_t> &cur, const int32_t *ids, int n, const int32_t *confs, PnConfChange *ch) {
  const int B = (int)cur.size();
  if (!ch) { pn_set_error("bad argument"); return -1; }
  if (pn_conf_set_check(B, ids, n, confs)) return -1;
  ch->next = cur; ch->touched.clear(); ch->rows.clear(); ch->in_conf = 0;
  std::vector<int32_t> slot((size_t)B, -1);            // conference -> its index in touched
  for (int i = 0; i < n; i++) {
    const int32_t was = cur[ids[i]], now = confs[i];
    if (was == now) continue;
    ch->next[ids[i]] = now;
    for (int32_t c : {was, now})
      if (c != PN_CONF_NONE && slot[c] < 0) { slot[c] = 0; ch->touched.push_back(c); }
  }
  std::sort(ch->touched.begin(), ch->touched.end());
  for (size_t k = 0; k < ch->touched.size(); k++) slot[ch->touched[k]] = (int32_t)k;
  std::vector<int32_t> count(ch->touched.size(), 0);
  for (int s = 0; s < B; s++) {
    const int32_t c = ch->next[s];
    if (c == PN_CONF_NONE) continue;
    ch->in_conf++;
    if (slot[c] >= 0) count[slot[c]]++;
  }
  for (size_t k = 0; k < count.size(); k++)
    if (count[k] > PN_CONF_MAX_MEMBERS) {
      pn_set_error("conference %d would have %d members: a conference holds at most %d", (int)ch->touched[k], (int)count[k], PN_CONF_MAX_MEMBERS);
      return -1;
    }
  ch->rows.assign(ch->touched.size() * PN_CONF_MAX_MEMBERS, -1);
  std::fill(count.begin(), count.end(), 0);
  for (int s = 0; s < B; s++) {                        // ascending s: every row comes out in ascending slot order
    const int32_t c = ch->next[s];
    if (c == PN_CONF_NONE || slot[c] < 0) continue;
    ch->rows[(size_t)slot[c] * PN_CONF_MAX_MEMBERS + count[slot[c]]++] = s;
  }
  return 0;
}
