// ssvio_amd/csrc/rectify.inc -- ssx_stereo_rectify, the common rectified camera of a raw stereo rig: rectify() of tools/rectify_model.py,
// statement for statement, in host f64.  Included by undistort.hip and by nothing else: that translation unit is compiled with
// -ffp-contract=off, so every operation here rounds on its own as the model's does (tests/test_rectify_abi.py: the model's bits), and
// ud_known_model is defined there.  No HIP call.

namespace {

const char* const UD_WHY_MODEL = "unknown lens model";
const char* const UD_WHY_FINITE = "a non-finite input";
const char* const UD_WHY_BASELINE = "the baseline is zero";
const char* const UD_WHY_ROTATION = "R is not a rotation: max|R R^T - I| > 1e-6";
const char* const UD_WHY_SIDE = "the right camera is not to the right of the left one (e1[0] <= 0)";
const char* const UD_WHY_AXES = "the optical axes lie along the baseline (|e3'|^2 < 1e-12)";

inline bool ud_all_finite(const double* v, int n)
{
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

// iR = S^T newK^-1 in closed form; in the third column the left-most product is taken first
inline void ud_rect_iR(const double S[9], double f, double cx, double cy, double iR[9])
{
  const double g = 1.0 / f;
  const double mx = -cx / f;
  const double my = -cy / f;
  for (int i = 0; i < 3; ++i) {
    iR[3 * i + 0] = S[0 + i] * g;
    iR[3 * i + 1] = S[3 + i] * g;
    const double a = S[0 + i] * mx;
    const double b = S[3 + i] * my;
    const double ab = a + b;
    iR[3 * i + 2] = ab + S[6 + i];
  }
}

// -> nullptr and *o filled, or the model's reason and *o untouched
const char* ud_rectify(const ssx_stereo_raw_rig& rig, ssx_stereo_rectified* o)
{
  for (int s = 0; s < 2; ++s)
    if (!ud_known_model(rig.cam[s].model)) return UD_WHY_MODEL;
  const double over[3] = {rig.f, rig.cx, rig.cy};
  bool fin = ud_all_finite(rig.R, 9) && ud_all_finite(rig.t, 3) && ud_all_finite(over, 3);
  for (int s = 0; s < 2; ++s) fin = fin && ud_all_finite(rig.cam[s].K, 4) && ud_all_finite(rig.cam[s].coeffs, 5);
  if (!fin) return UD_WHY_FINITE;
  const double* R = rig.R;
  const double* t = rig.t;
  double c[3];
  for (int i = 0; i < 3; ++i) {
    const double a0 = (-R[0 + i]) * t[0];
    const double a1 = (-R[3 + i]) * t[1];
    const double a2 = (-R[6 + i]) * t[2];
    const double a01 = a0 + a1;
    c[i] = a01 + a2;
  }
  const double c00 = c[0] * c[0], c11 = c[1] * c[1], c22 = c[2] * c[2];
  const double cc = c00 + c11;
  const double b = std::sqrt(cc + c22);
  if (b == 0.0) return UD_WHY_BASELINE;
  double worst = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double p0 = R[3 * i + 0] * R[3 * j + 0], p1 = R[3 * i + 1] * R[3 * j + 1], p2 = R[3 * i + 2] * R[3 * j + 2];
      const double p01 = p0 + p1;
      const double dot = p01 + p2;
      const double dev = std::fabs(dot - (i == j ? 1.0 : 0.0));
      if (dev > worst) worst = dev;
    }
  if (worst > 1e-6) return UD_WHY_ROTATION;
  double e1[3], e2[3], e3[3], e3p[3];
  for (int i = 0; i < 3; ++i) e1[i] = c[i] / b;
  if (e1[0] <= 0.0) return UD_WHY_SIDE;
  const double zm[3] = {0.0 + R[6], 0.0 + R[7], 1.0 + R[8]};
  const double d0 = zm[0] * e1[0], d1 = zm[1] * e1[1], d2 = zm[2] * e1[2];
  const double d01 = d0 + d1;
  const double d = d01 + d2;
  for (int i = 0; i < 3; ++i) {
    const double de = d * e1[i];
    e3p[i] = zm[i] - de;
  }
  const double q0 = e3p[0] * e3p[0], q1 = e3p[1] * e3p[1], q2 = e3p[2] * e3p[2];
  const double q01 = q0 + q1;
  const double n2 = q01 + q2;
  if (n2 < 1e-12) return UD_WHY_AXES;
  const double nn = std::sqrt(n2);
  for (int i = 0; i < 3; ++i) e3[i] = e3p[i] / nn;
  {
    const double a0 = e3[1] * e1[2], b0 = e3[2] * e1[1];
    const double a1 = e3[2] * e1[0], b1 = e3[0] * e1[2];
    const double a2 = e3[0] * e1[1], b2 = e3[1] * e1[0];
    e2[0] = a0 - b0; e2[1] = a1 - b1; e2[2] = a2 - b2;
  }
  ssx_stereo_rectified r;
  std::memset(&r, 0, sizeof r);
  for (int i = 0; i < 3; ++i) { r.R_l[i] = e1[i]; r.R_l[3 + i] = e2[i]; r.R_l[6 + i] = e3[i]; }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double p0 = r.R_l[3 * i + 0] * R[3 * j + 0], p1 = r.R_l[3 * i + 1] * R[3 * j + 1], p2 = r.R_l[3 * i + 2] * R[3 * j + 2];
      const double p01 = p0 + p1;
      r.R_r[3 * i + j] = p01 + p2;
    }
  const double* Kl = rig.cam[0].K;
  const double* Kr = rig.cam[1].K;
  double f = rig.f, cx = rig.cx, cy = rig.cy;
  if (f == 0.0) {
    const double sl = Kl[0] + Kl[1], sr = Kr[0] + Kr[1];
    const double s4 = sl + sr;
    f = s4 / 4.0;
  }
  if (cx == 0.0) { const double s2 = Kl[2] + Kr[2]; cx = s2 / 2.0; }
  if (cy == 0.0) { const double s2 = Kl[3] + Kr[3]; cy = s2 / 2.0; }
  r.newK[0] = f; r.newK[1] = f; r.newK[2] = cx; r.newK[3] = cy;
  r.baseline = b;
  for (int s = 0; s < 2; ++s) {
    r.cam[s].model = rig.cam[s].model;                               // (reserved stays 0: equal lenses are equal bytes)
    std::memcpy(r.cam[s].K, rig.cam[s].K, sizeof r.cam[s].K);
    std::memcpy(r.cam[s].coeffs, rig.cam[s].coeffs, sizeof r.cam[s].coeffs);
    ud_rect_iR(s == 0 ? r.R_l : r.R_r, f, cx, cy, r.cam[s].iR);
  }
  *o = r;
  return nullptr;
}

}  // namespace

extern "C" {

ssx_status ssx_stereo_rectify(const ssx_stereo_raw_rig* rig, ssx_stereo_rectified* out, char* why, int32_t why_cap)
{
  const char* reason = !rig ? "rig is null" : !out ? "out is null" : ud_rectify(*rig, out);
  if (why && why_cap > 0) {
    std::strncpy(why, reason ? reason : "", (size_t)why_cap);
    why[why_cap - 1] = '\0';
  }
  return reason ? SSX_ERR_INVALID_ARG : SSX_OK;
}

}  // extern "C"
