// libmembrane_hip.so host side, part of ms_api.cpp (included there, in this order: one translation unit): what the
// setters of the ring and rim modules check and derive the same way -- a plane's center and normal, its in-plane axes, a
// ring's external rows.  Each refuses through fail() with the setter's name in front, so every text is its caller's.
namespace {

// a plane's first refusal; its second is plane_frame's, and a setter may test arguments of its own between the two
int plane_finite(ms_ctx* c, const char* who, const double center[3], const double normal[3]) {
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(center[k]) || !std::isfinite(normal[k]))
      return fail(c, MS_ERR_INVALID, std::string(who) + ": center and normal must be finite");
  return MS_OK;
}

// the unit normal n of a finite normal, refused below |normal| = 1e-15, and on request the in-plane axes u, v
// (geometry/plane_ops.py:21-41, tilt_thetaB_contact_in.py:97-111: a trial axis off the normal, two degenerate fallbacks)
int plane_frame(ms_ctx* c, const char* who, const double normal[3], double n[3], double* u = nullptr, double* v = nullptr) {
  double nn = 0.0;
  for (int k = 0; k < 3; ++k) nn += normal[k] * normal[k];
  nn = std::sqrt(nn);
  if (!(nn >= 1e-15)) return fail(c, MS_ERR_INVALID, std::string(who) + ": a non-zero plane normal is required");
  for (int k = 0; k < 3; ++k) n[k] = normal[k] / nn;
  if (!u || !v) return MS_OK;
  double trial[3] = {1.0, 0.0, 0.0};
  if (std::fabs(n[0]) > 0.9) {
    trial[0] = 0.0;
    trial[1] = 1.0;
  }
  const double tn = trial[0] * n[0] + trial[1] * n[1] + trial[2] * n[2];
  for (int k = 0; k < 3; ++k) u[k] = trial[k] - tn * n[k];
  const double un = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int k = 0; k < 3; ++k) u[k] = un < 1e-15 ? (k == 0 ? 1.0 : 0.0) : u[k] / un;
  v[0] = n[1] * u[2] - n[2] * u[1];
  v[1] = n[2] * u[0] - n[0] * u[2];
  v[2] = n[0] * u[1] - n[1] * u[0];
  const double vn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  for (int k = 0; k < 3; ++k) v[k] = vn < 1e-15 ? (k == 1 ? 1.0 : 0.0) : v[k] / vn;
  return MS_OK;
}

// a ring's n external rows as library rows (iperm: external -> library) into out: each inside [0, nv) and listed once.
// seen holds nv zeros before the first ring; rings that must not share a row hand the same map on.  The two refusals
// read "<who>: <noun> row out of range" and "<who>: <a_noun> row is listed twice<twice_tail>"; c == nullptr: a host
// entry point without a context.
int ring_rows(ms_ctx* c, const char* who, const char* noun, const char* a_noun, int nv, const int32_t* iperm, int n,
              const int32_t* rows, std::vector<uint8_t>& seen, int32_t* out, const char* twice_tail = "") {
  for (int i = 0; i < n; ++i) {
    const int32_t r = rows[i];
    if (r < 0 || r >= nv) return fail(c, MS_ERR_INVALID, std::string(who) + ": " + noun + " row out of range");
    if (seen[(size_t)r])
      return fail(c, MS_ERR_INVALID, std::string(who) + ": " + a_noun + " row is listed twice" + twice_tail);
    seen[(size_t)r] = 1;
    out[i] = iperm[(size_t)r];
  }
  return MS_OK;
}

}  // namespace
