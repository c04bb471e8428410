// CPU-only sanitizer harness of the conference table's host rules (tests/test_conf_host.py builds it with
// g++ -DPN_NO_HIP -fsanitize=address,undefined, like g711_sanitize.cpp): pn_conf.h over exactly-sized heap buffers — tables of 0
// and 1 streams, the value check, a conference of exactly 32 and one of 33, ascending order for interleaved members, and changes
// that move streams between two full conferences.  Prints "ok" and exits 0.
#include "../../percepnet_amd/csrc/pn_model.cpp"          // pn_set_error / pn_last_error
#include "../../percepnet_amd/csrc/pn_conf.h"
#include <stdio.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "conf_sanitize: CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #c, pn_last_error()); return 1; } } while (0)

typedef std::vector<int32_t> V;

// every touched row of a change: the members of that conference in ch.next by the plain scan, ascending, -1 behind them
static bool rows_are_the_members(const PnConfChange &ch) {
  if (ch.rows.size() != ch.touched.size() * PN_CONF_MAX_MEMBERS) return false;
  for (size_t k = 0; k < ch.touched.size(); k++) {
    if (k && ch.touched[k] <= ch.touched[k - 1]) return false;
    V m(PN_CONF_MAX_MEMBERS, -7);
    const int n = pn_conf_members(ch.next, ch.touched[k], m.data());
    if (n > PN_CONF_MAX_MEMBERS) return false;
    for (int j = 0; j < PN_CONF_MAX_MEMBERS; j++) {
      if (ch.rows[k * PN_CONF_MAX_MEMBERS + j] != (j < n ? m[j] : -1)) return false;
      if (j && j < n && m[j] <= m[j - 1]) return false;
    }
  }
  int in = 0;
  for (int32_t c : ch.next) in += c != PN_CONF_NONE;
  return in == ch.in_conf;
}

int main() {
  static_assert(PN_CONF_NONE == -1 && PN_CONF_MAX_MEMBERS == 32, "the header's constants");
  PnConfChange ch;
  // a table of 0 streams: only the empty change exists
  { V cur;
    CHECK(pn_conf_change(cur, NULL, 0, NULL, &ch) == 0 && ch.next.empty() && ch.touched.empty() && ch.rows.empty() && ch.in_conf == 0);
    V id1 = {0}, c1 = {PN_CONF_NONE};
    CHECK(pn_conf_change(cur, id1.data(), 1, c1.data(), &ch) == -1);
    CHECK(pn_conf_list_check(NULL, 0, 0) == 0 && pn_conf_list_check(c1.data(), 1, 0) == 0);
    V c0 = {0};
    CHECK(pn_conf_list_check(c0.data(), 1, 0) == -1 && strstr(pn_last_error(), "at index 0:"));
    V none(PN_CONF_MAX_MEMBERS, -7);
    CHECK(pn_conf_members(cur, 0, none.data()) == 0 && none[0] == -7); }
  // a table of 1 stream: conference 0 of one member, and out again
  { V cur = {PN_CONF_NONE}, id = {0}, in = {0}, out = {PN_CONF_NONE}, bad = {1};
    CHECK(pn_conf_change(cur, id.data(), 1, in.data(), &ch) == 0 && ch.next == in && ch.touched == in && ch.in_conf == 1 && rows_are_the_members(ch));
    CHECK(ch.rows[0] == 0 && ch.rows[1] == -1);
    V cur1 = ch.next;
    CHECK(pn_conf_change(cur1, id.data(), 1, in.data(), &ch) == 0 && ch.touched.empty() && ch.next == cur1 && ch.in_conf == 1);   // no change: nothing touched
    CHECK(pn_conf_change(cur1, id.data(), 1, out.data(), &ch) == 0 && ch.next == out && ch.touched == in && ch.in_conf == 0 && rows_are_the_members(ch));
    CHECK(ch.rows[0] == -1);
    CHECK(pn_conf_change(cur, id.data(), 1, bad.data(), &ch) == -1 && strstr(pn_last_error(), "at index 0:"));
    CHECK(pn_conf_change(cur, id.data(), 1, NULL, &ch) == -1 && pn_conf_change(cur, NULL, 1, in.data(), &ch) == -1 && pn_conf_change(cur, id.data(), 1, in.data(), NULL) == -1); }
  // the value check names the first bad index
  { const int B = 6;
    V good = {PN_CONF_NONE, 0, 5, 5, PN_CONF_NONE, 3};
    CHECK(pn_conf_list_check(good.data(), 6, B) == 0 && pn_conf_list_check(good.data(), 0, B) == 0);
    CHECK(pn_conf_list_check(NULL, 3, B) == -1 && pn_conf_list_check(good.data(), -1, B) == -1 && pn_conf_list_check(good.data(), 6, -1) == -1);
    for (int at = 0; at < 6; at++)
      for (int32_t bad : {6, -2, 8000, (int32_t)0x80000000, (int32_t)0x7fffffff}) {
        V t(good);
        t[at] = bad;
        if (at < 5) t[5] = 77;                                 // a later bad one is not the one named
        CHECK(pn_conf_list_check(t.data(), 6, B) == -1);
        char want[32];
        snprintf(want, sizeof(want), "at index %d:", at);
        CHECK(strstr(pn_last_error(), want) != NULL);
      } }
  // the id rule first (distinct, in range), then the values
  { const int B = 5;
    V cur(B, PN_CONF_NONE), w = {1, 1, PN_CONF_NONE};
    { V t = {4, 0, 4}; CHECK(pn_conf_change(cur, t.data(), 3, w.data(), &ch) == -1 && strstr(pn_last_error(), "twice")); }
    { V t = {4, 5, 2}; CHECK(pn_conf_change(cur, t.data(), 3, w.data(), &ch) == -1 && strstr(pn_last_error(), "out of range")); }
    { V t = {4, -1, 2}; CHECK(pn_conf_change(cur, t.data(), 3, w.data(), &ch) == -1); }
    { V t = {4, 0, 2}, v = {1, 0, 5}; CHECK(pn_conf_change(cur, t.data(), 3, v.data(), &ch) == -1 && strstr(pn_last_error(), "at index 2:")); }
    { V t = {4, 0, 2}; CHECK(pn_conf_set_check(B, t.data(), 3, w.data()) == 0 && pn_conf_set_check(B, t.data(), 0, NULL) == 0); } }
  // interleaved members: conferences 70 (even slots below 64), 3 (the slots 1, 7, .., 79) and 0 (two slots far apart), handed over
  // in DESCENDING id order — the rows come out ascending
  const int B = 80;
  V table(B, PN_CONF_NONE);
  { V ids, confs;
    for (int s = B - 1; s >= 0; s--) {
      const int32_t c = s < 64 && s % 2 == 0 ? 70 : s % 6 == 1 ? 3 : (s == 5 || s == 77) ? 0 : PN_CONF_NONE;
      ids.push_back(s); confs.push_back(c);
    }
    CHECK(pn_conf_change(table, ids.data(), B, confs.data(), &ch) == 0 && rows_are_the_members(ch));
    CHECK((ch.touched == V{0, 3, 70}));
    CHECK(ch.rows[0] == 5 && ch.rows[1] == 77 && ch.rows[2] == -1 && ch.in_conf == 32 + 14 + 2);
    CHECK(ch.rows[32] == 1 && ch.rows[33] == 7 && ch.rows[32 + 13] == 79 && ch.rows[32 + 14] == -1);
    V m(PN_CONF_MAX_MEMBERS);
    CHECK(pn_conf_members(ch.next, 70, m.data()) == 32 && m[0] == 0 && m[31] == 62);                  // exactly the cap
    for (int j = 0; j < 32; j++) CHECK(ch.rows[2 * 32 + j] == 2 * j);
    table = ch.next; }
  // a 33rd member is refused, the message names the conference and its size, and nothing is decided
  { V id = {65}, c = {70};
    CHECK(pn_conf_change(table, id.data(), 1, c.data(), &ch) == -1);
    CHECK(strstr(pn_last_error(), "conference 70") && strstr(pn_last_error(), "33 members"));
    V m(PN_CONF_MAX_MEMBERS);
    CHECK(pn_conf_members(table, 70, m.data()) == 32);
    // one leaves, one joins, in one call: 32 after the change
    V id2 = {65, 0}, c2 = {70, PN_CONF_NONE};
    CHECK(pn_conf_change(table, id2.data(), 2, c2.data(), &ch) == 0 && rows_are_the_members(ch) && (ch.touched == V{70}));
    CHECK(ch.rows[0] == 2 && ch.rows[31] == 65); }
  // two full conferences: 70 (above) and 71 (32 of the free slots)
  { V ids, confs;
    for (int s = 0; s < B && (int)ids.size() < 32; s++)
      if (table[s] == PN_CONF_NONE) { ids.push_back(s); confs.push_back(71); }
    CHECK((int)ids.size() == 32);
    CHECK(pn_conf_change(table, ids.data(), 32, confs.data(), &ch) == 0 && rows_are_the_members(ch));
    table = ch.next;
    V m(PN_CONF_MAX_MEMBERS), q(PN_CONF_MAX_MEMBERS);
    CHECK(pn_conf_members(table, 70, m.data()) == 32 && pn_conf_members(table, 71, q.data()) == 32);
    // a stream moves from one full conference to the other: 33 there
    V id = {m[7]}, c = {71};
    CHECK(pn_conf_change(table, id.data(), 1, c.data(), &ch) == -1 && strstr(pn_last_error(), "conference 71") && strstr(pn_last_error(), "33 members"));
    // two streams swap: both stay at 32, both rows change and stay ascending
    V id2 = {m[7], q[20]}, c2 = {71, 70};
    CHECK(pn_conf_change(table, id2.data(), 2, c2.data(), &ch) == 0 && rows_are_the_members(ch) && (ch.touched == V{70, 71}));
    CHECK(ch.next[m[7]] == 71 && ch.next[q[20]] == 70 && ch.in_conf == 80);
    CHECK(pn_conf_members(ch.next, 70, m.data()) == 32 && pn_conf_members(ch.next, 71, q.data()) == 32);
    // a whole conference dissolves: its row is all -1
    V all, none;
    for (int j = 0; j < 32; j++) { all.push_back(m[j]); none.push_back(PN_CONF_NONE); }
    V cur = ch.next;
    CHECK(pn_conf_change(cur, all.data(), 32, none.data(), &ch) == 0 && (ch.touched == V{70}) && rows_are_the_members(ch));
    for (int j = 0; j < 32; j++) CHECK(ch.rows[j] == -1); }
  puts("ok");
  return 0;
}
