// The rules of the C-ABI's host side that need no GPU, each stated once — HIP-free (builds with -DPN_NO_HIP), checked on the CPU by
// tests/c/host_sanitize.cpp under the sanitizers: what a list of stream ids must be, the header verdicts every state record shares
// (stream-state records here, rate-state records in pn_rate_design.h), and the all-or-nothing walk over a batch of records.
#pragma once
#include "pn_common.h"
#include "../../include/percepnet_hip.h"
#include <string.h>
#include <string>
#include <vector>

// ---- a list of stream ids -----------------------------------------------------------------------------------------------------
// ids[0..n) name streams of a batch of B.  Refused, in this order, with -1 and pn_last_error set: a negative count or a list without
// a pointer; a `distinct` list longer than B; then, in list order, an id out of range and (when `distinct`) an id seen before.
// n == 0 is a legal list.  distinct: where the streams advance or are written (duplicates are legal where they are only reset or
// read).  mark (optional, used when `distinct`): a caller-owned vector that is left as B flags, 1 for the ids listed before the
// verdict and 0 for every other stream — a caller on the frame path keeps one, so that its checks allocate nothing.
static inline int pn_ids_check(int B, const int32_t *ids, int n, bool distinct, std::vector<uint8_t> *mark = NULL) {
  if (n < 0 || (n > 0 && !ids)) { pn_set_error("bad argument"); return -1; }
  if (distinct && n > B) { pn_set_error("%d stream ids in a context of %d", n, B); return -1; }
  std::vector<uint8_t> own;
  std::vector<uint8_t> &seen = mark ? *mark : own;
  if (distinct) seen.assign((size_t)B, 0);
  for (int i = 0; i < n; i++) {
    if (ids[i] < 0 || ids[i] >= B) { pn_set_error("stream id %d out of range [0, %d)", ids[i], B); return -1; }
    if (distinct && seen[ids[i]]++) { pn_set_error("stream id %d listed twice", ids[i]); return -1; }
  }
  return 0;
}

// ---- state records --------------------------------------------------------------------------------------------------------------
static inline uint32_t pn_le32(const unsigned char *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
// The verdicts every record shares, in their order: too short to hold the 16 bytes they read (PN_SS_BAD_SIZE; the caller, who knows
// what a record of its kind has, words that one), then the magic, then the version.  name: "stream-state" / "rate-state".
static inline int pn_record_header_check(const unsigned char *r, size_t bytes, uint32_t magic, uint32_t version, const char *name) {
  if (bytes < 16) return PN_SS_BAD_SIZE;
  if (pn_le32(r) != magic) { pn_set_error("not a %s record (magic 0x%08x)", name, pn_le32(r)); return PN_SS_BAD_MAGIC; }
  if (pn_le32(r + 4) != version) { pn_set_error("%s record version %u, this library reads %d", name, pn_le32(r + 4), (int)version); return PN_SS_BAD_VERSION; }
  return PN_SS_OK;
}
// All or nothing: the header of every one of the n records of rec_bytes at h_records, before anything is launched.  check(record,
// bytes) is the record kind's own check (0 = accepted, pn_last_error says why not).
template <class Check>
static inline int pn_records_check(const void *h_records, int n, size_t rec_bytes, Check check) {
  for (int i = 0; i < n; i++)
    if (check(static_cast<const char *>(h_records) + (size_t)i * rec_bytes, rec_bytes)) {
      std::string why = pn_last_error();
      pn_set_error("record %d refused: %s", i, why.c_str());
      return -1;
    }
  return 0;
}

// ---- per-stream state records (pn_stream_state.hip; layout in include/percepnet_hip.h) ------------------------------
// The header words a context writes (export) and expects (import; word 3, the source's nn_mode, is not compared).
static inline void ss_header(uint32_t hdr[16], const unsigned char digest[32], int nn_mode) {
  memset(hdr, 0, 16 * sizeof(uint32_t));
  hdr[0] = PN_STREAM_STATE_MAGIC; hdr[1] = PN_STREAM_STATE_VERSION; hdr[2] = PN_STREAM_STATE_BYTES; hdr[3] = (uint32_t)nn_mode;
  memcpy(&hdr[4], digest, 32);
}
// host twin of the import kernel's check (pn_stream_state.hip ss_check), same order of verdicts: the shared ones, then the size,
// then the model digest
static inline int ss_check_host(const void *record, size_t bytes, const unsigned char digest[32]) {
  const unsigned char *r = static_cast<const unsigned char *>(record);
  const int v = pn_record_header_check(r, bytes, PN_STREAM_STATE_MAGIC, PN_STREAM_STATE_VERSION, "stream-state");
  if (v == PN_SS_BAD_SIZE) pn_set_error("stream-state record of %zu bytes: a record has %d", bytes, PN_STREAM_STATE_BYTES);
  if (v) return v;
  if (pn_le32(r + 8) != PN_STREAM_STATE_BYTES || bytes != PN_STREAM_STATE_BYTES) {
    pn_set_error("stream-state record of %zu bytes (header: %u), a record has %d", bytes, pn_le32(r + 8), PN_STREAM_STATE_BYTES);
    return PN_SS_BAD_SIZE;
  }
  if (memcmp(r + 16, digest, 32)) { pn_set_error("stream-state record written under another model (pn_model_digest differs)"); return PN_SS_BAD_MODEL; }
  return PN_SS_OK;
}
