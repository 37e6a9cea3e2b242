// Device-only helpers of the modules that order a ring of vertices by angle at every evaluation (ms_thetab.hip,
// ms_rimmatch.hip); included inside a .hip file only.
//
// The ordering is np.argsort of the rows' angles about the plane's center, and it depends on the positions handed to the
// evaluation, so it is not a table the host can build once: one workgroup keeps the ring's angles in LDS and ranks them
// by counting -- rank_i = #{j : (key_j, j) < (key_i, i)}, a strict total order on doubles, ties broken by the row's
// number in its table.  That needs no padding to a power of two, handles every n from 1 up and reads LDS as a broadcast
// (every lane the same j).  The angle itself stays with each caller: the two modules do not take atan2 of the same double.
#pragma once
#include "ms_stream_dev.h"

namespace ms {
namespace {

// p - center without its component along the normal; A has center and normal (the unit normal)
template <class A>
__device__ __forceinline__ P3 ring_in_plane(const A& a, const P3& p) {
  const double rx = p.x - a.center[0], ry = p.y - a.center[1], rz = p.z - a.center[2];
  const double rn = rx * a.normal[0] + ry * a.normal[1] + rz * a.normal[2];
  return P3{rx - rn * a.normal[0], ry - rn * a.normal[1], rz - rn * a.normal[2]};
}

// key[0 .. n) -> ord: ord[q] is the table index of the q-th smallest key.  Every thread of the workgroup calls it, having
// written key[i] and ord[i] = i for its items (so every slot holds an index of the ring even if a non-finite key breaks
// the ranks); key and ord are in LDS, and ord is complete for the whole workgroup on return.
__device__ __forceinline__ void ring_rank(const double* key, int* ord, int n) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += LB) {
    const double ki = key[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double kj = key[j];
      rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
    ord[rank] = i;  // (rank < n: at most n - 1 rows come before row i)
  }
  __syncthreads();
}

// the arc-length weight 1/2 (|p_next - p| + |p - p_prev|) of slot q (position p) of an ordered closed ring of n rows;
// row_of(s) is the row in slot s; A has x, d, alpha and vflags
template <class A, class RowOf>
__device__ __forceinline__ double ring_arc_weight(const A& a, int n, int q, const P3& p, RowOf row_of) {
  const P3 pp = row_at(a, row_of(q == 0 ? n - 1 : q - 1));
  const P3 pn = row_at(a, row_of(q + 1 == n ? 0 : q + 1));
  return 0.5 * (len3(pn.x - p.x, pn.y - p.y, pn.z - p.z) + len3(p.x - pp.x, p.y - pp.y, p.z - pp.z));
}

}  // namespace
}  // namespace ms
