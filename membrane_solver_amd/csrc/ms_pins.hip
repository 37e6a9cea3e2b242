// pin_to_plane / pin_to_circle on the device: the enforcement program (modules/constraints/pin_to_plane.py and
// pin_to_circle.py enforce_constraint) and the project lane's gradient pass (the sparse rows of
// constraint_gradients_rows_array removed from G, and from the volume row GC, at the pinned rows).
//
// Both kernels are ONE workgroup: the pinned rows are a rim (O(sqrt(nf)) vertices).  Stages run in order with a
// workgroup barrier between them; group sums are a fixed-order tree in LDS (thread t adds members t, t+PB, ... in
// order, then a halving tree), so a run is bitwise reproducible.
#include "ms_internal.h"
#include "ms_pins_dev.h"

namespace ms {
namespace {

using pin_dev::PB;

__global__ __launch_bounds__(PB) void k_pin_enforce(PinEnforceArgs a) {
  __shared__ double red[3][PB];
  pin_dev::pin_enforce_body(a, red);
}

__global__ __launch_bounds__(PB) void k_pin_grad(PinGradArgs a) {
  __shared__ double red[3][PB];
  pin_dev::pin_grad_body(a, red);
}

}  // namespace

// record: the one-workgroup interpreter runs the program as a record of its pack (stream order is the pack's order);
// otherwise whatever is recorded is launched first
hipError_t launch_pin_enforce(const PinEnforceArgs& a, hipStream_t s, bool record) {
  if (a.n_stages <= 0) return hipSuccess;
  if (ExecRecorder* r = exec_find(s)) {
    if (record) return r->push(CK_PIN_ENFORCE, 0, 0, 0, 1, 0, sizeof(double) * 3 * PB, &a, sizeof(a));
    if (const hipError_t e = r->flush(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_pin_enforce, dim3(1), dim3(PB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pin_grad(const PinGradArgs& a, hipStream_t s, bool record) {
  if (a.n_grad <= 0 && a.n_avg <= 0) return hipSuccess;
  if (ExecRecorder* r = exec_find(s)) {
    if (record) return r->push(CK_PIN_GRAD, 0, 0, 0, 1, 0, sizeof(double) * 3 * PB, &a, sizeof(a));
    if (const hipError_t e = r->flush(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_pin_grad, dim3(1), dim3(PB), 0, s, a);
  return hipGetLastError();
}

}  // namespace ms
