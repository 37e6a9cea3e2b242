// ASan/UBSan run of ms_leaflet_absent_flags_host (host code only, no context, no GPU): the flag update of
// ms_set_leaflet_absent -- the absence bit through the vertex permutation, every other bit kept -- over empty, identity,
// reversed, set, cleared (NULL) and out-of-range inputs.  The arrays are allocated at exactly nv bytes / entries, so a
// read or write past them is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "membrane_hip.h"
#include "ms_test_hooks.h"

static const uint8_t ABSENT = 32;

static int run(const char* what, int nv, const std::vector<int32_t>& perm_v, const std::vector<uint8_t>* absent_v,
               const std::vector<uint8_t>& flags_v, int want_rc, int want_state) {
  // heap blocks of exactly the documented room (new[] so the redzones sit right behind them)
  int32_t* perm = new int32_t[nv > 0 ? nv : 1];
  uint8_t* absent = absent_v ? new uint8_t[nv > 0 ? nv : 1] : nullptr;
  uint8_t* flags = new uint8_t[nv > 0 ? nv : 1];
  if (nv > 0) {
    memcpy(perm, perm_v.data(), sizeof(int32_t) * nv);
    memcpy(flags, flags_v.data(), nv);
    if (absent) memcpy(absent, absent_v->data(), nv);
  }
  int state = -1;
  const int rc = ms_leaflet_absent_flags_host(nv, perm, absent, flags, &state);
  int bad = rc != want_rc;
  if (rc == MS_OK) {
    bad |= state != want_state;
    for (int i = 0; i < nv && !bad; ++i) {
      const bool on = absent && absent[perm[i]];
      bad |= (flags[i] & (uint8_t)~ABSENT) != (flags_v[i] & (uint8_t)~ABSENT);  // the other bits are kept
      bad |= ((flags[i] & ABSENT) != 0) != on;
    }
  }
  printf("%-34s nv=%d rc=%d (want %d) state=%d (want %d) %s\n", what, nv, rc, want_rc, state, want_state, bad ? "BAD" : "ok");
  delete[] perm;
  delete[] absent;
  delete[] flags;
  return bad;
}

int main() {
  int bad = 0;
  const int nv = 9;
  std::vector<int32_t> id(nv), rev(nv);
  for (int i = 0; i < nv; ++i) {
    id[i] = i;
    rev[i] = nv - 1 - i;
  }
  std::vector<uint8_t> none(nv, 0), some(nv, 0), all(nv, 1), plain(nv), carrying(nv);
  some[0] = some[3] = 1;
  some[8] = 7;  // (any non-zero byte selects the row)
  for (int i = 0; i < nv; ++i) {
    plain[i] = (uint8_t)(i % 32);                // every other bit pattern below the absence bit, none carrying it
    carrying[i] = (uint8_t)((i % 32) | ABSENT);  // ... and all carrying it
  }
  bad |= run("nv = 0", 0, {}, &none, {}, MS_OK, 0);
  bad |= run("no row, nothing set before", nv, id, &none, plain, MS_OK, 0);
  bad |= run("NULL clears nothing", nv, id, nullptr, plain, MS_OK, 0);
  bad |= run("NULL clears every row", nv, id, nullptr, carrying, MS_OK, 1);
  bad |= run("some rows", nv, id, &some, plain, MS_OK, 3);
  bad |= run("some rows, reversed permutation", nv, rev, &some, plain, MS_OK, 3);
  bad |= run("every row", nv, rev, &all, plain, MS_OK, 3);
  bad |= run("every row, already set", nv, id, &all, carrying, MS_OK, 2);
  bad |= run("some rows replace every row", nv, rev, &some, carrying, MS_OK, 3);
  std::vector<int32_t> badperm = id;
  badperm[2] = 40;
  bad |= run("permutation out of range", nv, badperm, &some, plain, MS_ERR_INVALID, -1);
  badperm[2] = -1;
  bad |= run("permutation negative", nv, badperm, &some, plain, MS_ERR_INVALID, -1);
  {
    int state = 0;
    uint8_t f[1] = {0};
    bad |= ms_leaflet_absent_flags_host(-1, id.data(), none.data(), f, &state) != MS_ERR_INVALID;
    bad |= ms_leaflet_absent_flags_host(nv, nullptr, none.data(), f, &state) != MS_ERR_INVALID;
    bad |= ms_leaflet_absent_flags_host(nv, id.data(), none.data(), nullptr, &state) != MS_ERR_INVALID;
    std::vector<uint8_t> fl = plain;
    bad |= ms_leaflet_absent_flags_host(nv, id.data(), some.data(), fl.data(), nullptr) != MS_OK;  // (state is optional)
  }
  printf(bad ? "FAILED\n" : "all clean\n");
  return bad;
}
