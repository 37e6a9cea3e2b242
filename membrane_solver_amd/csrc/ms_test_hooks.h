// Entry points that exist for tests and sanitizer runs only: exported by libmembrane_hip.so, no part of the public
// interface (include/membrane_hip.h).
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// The flag update ms_set_leaflet_absent runs, on the host and without a context: flags[i] of library row i takes the
// absence bit (32) from absent[perm[i]] -- from no row when absent is NULL -- and keeps its other bits; *state = 1 when
// some flag changed | 2 when some row carries the bit.  MS_ERR_INVALID on a permutation entry outside [0, nv).
int ms_leaflet_absent_flags_host(int nv, const int32_t* perm /* nv */, const uint8_t* absent /* nv or NULL */,
                                 uint8_t* flags /* nv, in/out */, int* state);

#ifdef __cplusplus
}
#endif
